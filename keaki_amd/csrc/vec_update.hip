// vec_update: change k evaluations of a committed vector and move the commitment and ALL d opening proofs along, without the vector.
//
// Notation: d = 2^log2d, w = omega_d, P_k = srs[k] = [tau^k]_1, A(X) = X^d - 1, c_i = w^i / d, pi_j the opening at w^j.
// Two tables of d G1 points per (SRS, d), each one size-d group DFT with root w^-1 (g1_dif_run: the stage machinery of fft_g1.hip):
//   S_i = sum_k w^(-ik) P_k,              a_i = w^-i S_i       = [A(tau) / (tau - w^i)]_1          ([L_i(tau)]_1 = c_i a_i)
//   T_i = sum_k (d-1-k) w^(-ik) P_k,      u_i = (w^-i / d) T_i = [(L_i(tau) - 1) / (tau - w^i)]_1
// and two scalar tables: pw_i = w^-i and e_t = 1 / (w^t - 1) (t = 1 .. d-1; Fermat per lane), so that 1 / (w^i - w^j) = w^-j e_((i-j) mod d).
// For the change list (i_t, delta_t), evaluation i_t += delta_t:
//   com'  = com  + sum_t (delta_t c_(i_t)) a_(i_t)
//   pi_j' = pi_j + sum_{t: i_t != j} s_tj a_(i_t)  -  (sum_{t: i_t != j} s_tj) a_j  +  (sum_{t: i_t = j} delta_t) u_j,    s_tj = delta_t c_(i_t) w^-j e_((i_t - j) mod d)
// (polynomial identities in tau: they hold for every SRS; duplicates add). tests/vec_update_model.py is this file over Z_r.
//
// The proof kernel, one lane per proof j, runs the list in passes of at most UPD_K_PASS entries. The bases a_(i_t) of a pass are shared by all
// lanes, the scalars s_tj are per lane: interleaved Straus over GLV halves. k_upd_prep writes, per entry, the 15 TRUE affine multiples
// m a_(i_t) (m = 1 .. 15, 128-byte rows (y, x, beta x) in the lazy limbs, as the FK23 ladders' tables) and the wave-uniform header (i_t, delta_t,
// delta_t c_(i_t)); a lane splits every s_tj into two 127-bit halves (8 words per entry in LDS, lane-strided), and runs ONE chain of
// 32 x 4 doublings with 2 mixed additions per entry and window (unsigned 4-bit digits, read straight out of the halves). The issue's sketch
// was 254 doublings + 64 additions per base without the endomorphism; the split costs the same 64 additions and half the doublings, and the
// table row already carries beta x. The lane's own terms -(sum s) a_j and (sum delta) u_j have per-lane bases: they go through the ladder of
// the FK23 kernels (jac_scalar_mul_gtab_u29, workspace fk_tab), one instance in a two-trip loop. Every addition is complete: j29_madd reports
// equal / opposite operands, the four results meet in jac_add.
#include "jac29.hip.h"
#include "internal.h"
#include "kzg_fr.hip.h"

namespace bn254 {

// the wave-uniform data of one pass (device memory, read through a uniform address)
struct UpdHdr {
  u32 idx[keaki_internal::UPD_K_PASS];       // i_t; 0xFFFFFFFF: an index outside the domain (the _dev form cannot refuse it: the entry does nothing)
  u32 skip[keaki_internal::UPD_K_PASS];      // a_(i_t) is the identity (or the index is outside): no window table, no additions
  Fr sc[keaki_internal::UPD_K_PASS];         // delta_t c_(i_t)
  Fr delta[keaki_internal::UPD_K_PASS];
};
constexpr u32 UPD_ROW_WORDS = 32, UPD_ROWS = 16;      // window table of one base: row m - 1 = m a, 15 rows used

// e[t] = 1 / (w^t - 1), t >= 1; e[0] = 0 (never read). pw[i] = w^-i, so w^t = pw[d - t].
static __global__ void __launch_bounds__(64) k_upd_etab(const Fr* __restrict__ pw, u32 d, Fr* __restrict__ e) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d) return;
  e[t] = t ? fr_inv(fp_sub<FrParams>(pw[d - t], fp_one<FrParams>())) : fp_zero<FrParams>();
}
// s[k] = P_k, w[k] = (d - 1 - k) P_k  (the weights are below 2^27: plain double-and-add)
static __global__ void __launch_bounds__(64) k_upd_load(const G1Aff* __restrict__ srs, u32 d, G1Jac* __restrict__ s, G1Jac* __restrict__ w) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  const G1Aff p = srs[k];
  s[k] = jac_from_aff(p);
  const u32 m = d - 1 - k;
  G1Jac acc = jac_inf<Fq>();
#pragma unroll 1
  for (int b = 31 - __clz((int)(m | 1u)); b >= 0; b--) {
    acc = jac_dbl(acc);
    if ((m >> b) & 1u) acc = jac_add_mixed(acc, p);
  }
  w[k] = acc;
}
KDEV u32 upd_brev(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
KDEV uint4* upd_slot(uint4* tab, u32 lane, u32 first) { return tab ? tab + (size_t)(lane - first) * GTAB_UINT4_PER_LANE : nullptr; }
template <bool GT>
KDEV G1Jac upd_scalar_mul(const G1Jac& p, const Fr& k_mont, uint4* slot) {
  if constexpr (GT) return jac_scalar_mul_gtab_u29(p, k_mont, slot);
  else return jac_scalar_mul_u29(p, k_mont);
}
// lane q < 2d over the transforms [S | T] (bit-reversed positions): a[i] = affine(pw_i S_i), u[i] = affine(pw_i / d T_i), i = brev(q mod d)
template <bool GT>
static __global__ void __launch_bounds__(64) k_upd_finish(const G1Jac* __restrict__ st, const Fr* __restrict__ pw, Fr inv_d, u32 log2d, G1Aff* __restrict__ a,
                                                          G1Aff* __restrict__ u, uint4* __restrict__ tab, u32 first) {
  const u32 q = first + blockIdx.x * blockDim.x + threadIdx.x, d = 1u << log2d;
  if (q >= 2 * d) return;
  const u32 part = q >= d ? 1u : 0u, i = upd_brev(q - part * d, log2d);
  Fr sc = pw[i];
  if (part) sc = fp_mul<FrParams>(sc, inv_d);
  const G1Aff r = jac_to_aff(upd_scalar_mul<GT>(st[q], sc, upd_slot(tab, q, first)));
  if (part) u[i] = r; else a[i] = r;
}

// ---- one pass: header and window tables -----------------------------------------------------------------------------------------------------
// block t < cnt: lane 0 writes the header of entry t, lanes m = 1 .. 15 the row of m a_(i_t)
static __global__ void __launch_bounds__(64) k_upd_prep(const G1Aff* __restrict__ a, const Fr* __restrict__ pw, Fr inv_d, u32 d, const u32* __restrict__ idx,
                                                        const Fr* __restrict__ deltas, u32 cnt, UpdHdr* __restrict__ hdr, u32* __restrict__ wtab) {
  const u32 t = blockIdx.x, m = threadIdx.x;
  if (t >= cnt || m > 15) return;
  const u32 it = idx[t];
  const bool bad = it >= d;
  const G1Aff base = bad ? aff_inf<Fq>() : a[it];
  const bool skip = aff_is_inf(base);
  if (m == 0) {
    hdr->idx[t] = bad ? 0xFFFFFFFFu : it;
    hdr->skip[t] = skip ? 1u : 0u;
    hdr->delta[t] = bad ? fp_zero<FrParams>() : deltas[t];
    hdr->sc[t] = bad ? fp_zero<FrParams>() : fp_mul<FrParams>(fp_mul<FrParams>(deltas[t], pw[(d - it) & (d - 1)]), inv_d);
    return;
  }
  if (skip) return;
  G1Jac acc = jac_inf<Fq>();
#pragma unroll 1
  for (int b = 3; b >= 0; b--) {
    acc = jac_dbl(acc);
    if ((m >> b) & 1u) acc = jac_add_mixed(acc, base);
  }
  const G1Aff r = jac_to_aff(acc);                  // m < r on a group of prime order: never the identity
  const U29 x = u29_from_fq(r.x), y = u29_from_fq(r.y);
  u32* row = wtab + ((size_t)t * UPD_ROWS + (m - 1u)) * UPD_ROW_WORDS;
  st9(row, y);
  st9(row + 9, x);
  st9(row + 18, u29_mul(x, u29_const(GlvParams::BETA29)));
}

// ---- the proof kernel ---------------------------------------------------------------------------------------------------------------------------
template <bool GT>
static __global__ void __launch_bounds__(64) k_upd_proofs(const G1Aff* __restrict__ a, const G1Aff* __restrict__ u, const Fr* __restrict__ e,
                                                          const Fr* __restrict__ pw, const UpdHdr* __restrict__ hdr, const u32* __restrict__ wtab, u32 cnt, u32 d,
                                                          G1Aff* __restrict__ proofs, uint4* __restrict__ tab, u32 first) {
  // the GLV halves of this wave's scalars: word w of entry t of lane l at ((t * 8 + w) * 64 + l); words 0..3 = |k1| (sign in bit 127), 4..7 = |k2|
  __shared__ u32 ks[keaki_internal::UPD_K_PASS * 8 * 64];
  const u32 j = first + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d) return;
  u32* mine = ks + threadIdx.x;
  const Fr wj = pw[j];
  Fr ssum = fp_zero<FrParams>(), dsum = fp_zero<FrParams>();
#pragma unroll 1
  for (u32 t = 0; t < cnt; t++) {
    const u32 it = hdr->idx[t];
    u32 k1[5], k2[5];
#pragma unroll
    for (int w = 0; w < 5; w++) k1[w] = k2[w] = 0;
    bool n1 = false, n2 = false;
    if (it == j) {
      dsum = fp_add<FrParams>(dsum, hdr->delta[t]);
    } else {
      const Fr s = fp_mul<FrParams>(fp_mul<FrParams>(hdr->sc[t], wj), e[(it - j) & (d - 1)]);
      ssum = fp_add<FrParams>(ssum, s);
      if (!hdr->skip[t]) {
        u32 k[8];
        fp_from_mont<FrParams>(k, s);
        glv_decompose(k, k1, n1, k2, n2);
      }
    }
    k1[3] |= n1 ? 0x80000000u : 0u;
    k2[3] |= n2 ? 0x80000000u : 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      mine[(t * 8 + w) * 64] = k1[w];
      mine[(t * 8 + 4 + w) * 64] = k2[w];
    }
  }
  U29 zero;
#pragma unroll
  for (int i = 0; i < 9; i++) zero.l[i] = 0;
  J29 acc;
  acc.x = zero; acc.y = zero; acc.z = zero;
  bool empty = true;
#pragma unroll 1
  for (int w = 31; w >= 0; w--) {
    if (!empty) { acc = j29_dbl(acc); acc = j29_dbl(acc); acc = j29_dbl(acc); acc = j29_dbl(acc); }
#pragma unroll 1
    for (u32 t = 0; t < cnt; t++) {
      if (hdr->skip[t]) continue;
#pragma unroll 1
      for (u32 which = 0; which < 2; which++) {
        const u32* half = mine + (t * 8 + which * 4) * 64;
        const u32 top = half[3 * 64];
        u32 mag = ((w >= 24 ? top : half[(w >> 3) * 64]) >> ((w & 7) * 4)) & 15u;
        if (w == 31) mag &= 7u;
        if (mag) {
          const u32* row = wtab + ((size_t)t * UPD_ROWS + (mag - 1u)) * UPD_ROW_WORDS;
          const U29 ex = ld9(row + (which ? 18 : 9));
          const U29 y = ld9(row);
          const U29 ey = (top >> 31) ? u29_sub(zero, y, Q29::K4) : y;
          if (empty) {
            acc.x = ex; acc.y = ey; acc.z = u29_one();
            empty = false;
          } else {
            int special;
            acc = j29_madd(acc, ex, ey, special);
            if (special == 1) acc = j29_dbl(acc);
            if (special == 2) empty = true;
          }
        }
      }
    }
  }
  G1Jac r = jac_from_aff(proofs[j]);
  if (!empty) r = jac_add(r, j29_to_sat(acc));
  // the lane's own terms: -(sum s) a_j and (sum delta) u_j, one instance of the per-lane ladder
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    const Fr raw = q ? dsum : ssum;
    const G1Aff base = q ? u[j] : a[j];
    if (fp_is_zero<FrParams>(raw) || aff_is_inf(base)) continue;
    const Fr sc = q ? raw : fp_neg<FrParams>(raw);
    r = jac_add(r, upd_scalar_mul<GT>(jac_from_aff(base), sc, upd_slot(tab, j, first)));
  }
  proofs[j] = jac_to_aff(r);
}

// ---- the commitment: k scalar-mults and a sum (not hot) -------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(64) k_upd_com_terms(const G1Aff* __restrict__ a, const Fr* __restrict__ pw, Fr inv_d, u32 d, const u32* __restrict__ idx,
                                                             const Fr* __restrict__ deltas, u32 n, G1Jac* __restrict__ terms) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 it = idx[t];
  if (it >= d) { terms[t] = jac_inf<Fq>(); return; }
  const Fr sc = fp_mul<FrParams>(fp_mul<FrParams>(deltas[t], pw[(d - it) & (d - 1)]), inv_d);
  terms[t] = jac_scalar_mul_u29(jac_from_aff(a[it]), sc);
}
// com <- normalised(com + sum of the n terms): lane l sums the terms l, l + 64, .. into terms[l], lane 0 closes
static __global__ void __launch_bounds__(64) k_upd_com_sum(G1Jac* __restrict__ terms, u32 n, G1Jac* __restrict__ com) {
  const u32 l = threadIdx.x;
  if (l < n) {
    G1Jac acc = terms[l];
    for (u32 i = l + 64; i < n; i += 64) acc = jac_add(acc, terms[i]);
    terms[l] = acc;
  }
  __syncthreads();
  if (l) return;
  G1Jac acc = *com;
  for (u32 i = 0; i < n && i < 64; i++) acc = jac_add(acc, terms[i]);
  if (jac_is_inf(acc)) { *com = jac_inf<Fq>(); return; }
  const G1Aff r = jac_to_aff(acc);
  *com = {r.x, r.y, fq_one()};
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

// a (d affine) | u (d affine) | pw (d Fr) | e (d Fr)
size_t upd_table_bytes(uint32_t log2d) { return ((size_t)192) << log2d; }
namespace {
struct UpdTab { const G1Aff *a, *u; const Fr *pw, *e; };
UpdTab upd_view(const void* d_tab, uint32_t log2d) {
  const size_t d = (size_t)1 << log2d;
  const char* b = (const char*)d_tab;
  return {(const G1Aff*)b, (const G1Aff*)(b + d * 64), (const Fr*)(b + d * 128), (const Fr*)(b + d * 160)};
}
// launch(tab, first, lanes) over `total` lanes of a per-lane-ladder kernel, in pieces that fit the ladders' table workspace
template <class L>
void upd_ladder_launches(keaki_hip_ctx* ctx, u32 total, L launch) {
  u32 per = 0;
  uint4* tab = (uint4*)ladder_workspace(ctx, total, &per);
  if (!tab) { launch((uint4*)nullptr, 0u, total); return; }
  for (u32 first = 0; first < total; first += per) launch(tab, first, std::min(per, total - first));
}
}  // namespace

// Builds the update tables of (srs, d) at d_tab (upd_table_bytes). Workspace: 2d Jacobian points (ctx->vu_work).
keaki_status upd_tables_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2d, const uint64_t* omega_d_inv, const uint64_t* inv_d, void* d_tab) {
  const u32 d = 1u << log2d;
  const UpdTab t = upd_view(d_tab, log2d);
  ST_TRY(reserve(ctx, ctx->vu_work, (size_t)2 * d * sizeof(G1Jac)));
  G1Jac* s = (G1Jac*)ctx->vu_work.p;
  Fr invd;
  memcpy(&invd, inv_d, 32);
  hipStream_t st = ctx->stream;
  fr_powers_run(ctx, omega_d_inv, d, (void*)t.pw);
  hipLaunchKernelGGL(k_upd_etab, dim3(cdiv(d, 64)), dim3(64), 0, st, t.pw, d, (Fr*)t.e);
  hipLaunchKernelGGL(k_upd_load, dim3(cdiv(d, 64)), dim3(64), 0, st, (const G1Aff*)d_srs, d, s, s + d);
  ST_TRY(g1_dif_run(ctx, s, log2d, t.pw));
  ST_TRY(g1_dif_run(ctx, s + d, log2d, t.pw));
  upd_ladder_launches(ctx, 2 * d, [&](uint4* tab, u32 first, u32 cnt) {
    if (tab) hipLaunchKernelGGL(k_upd_finish<true>, dim3(cdiv(cnt, 64)), dim3(64), 0, st, (const G1Jac*)s, t.pw, invd, log2d, (G1Aff*)t.a, (G1Aff*)t.u, tab, first);
    else hipLaunchKernelGGL(k_upd_finish<false>, dim3(cdiv(cnt, 64)), dim3(64), 0, st, (const G1Jac*)s, t.pw, invd, log2d, (G1Aff*)t.a, (G1Aff*)t.u, tab, first);
  });
  return launch_check(ctx, "upd_tables");
}

// The update itself, everything on the device and in stream order. d_idx: k u32, d_deltas: k Fr, d_com: normalised Jacobian in / out or null,
// d_proofs: d affine in / out or null. k >= 1.
keaki_status upd_apply_run(keaki_hip_ctx* ctx, const void* d_tab, uint32_t log2d, const uint64_t* inv_d, const void* d_idx, const void* d_deltas, size_t k,
                           void* d_com, void* d_proofs) {
  const u32 d = 1u << log2d;
  const UpdTab t = upd_view(d_tab, log2d);
  Fr invd;
  memcpy(&invd, inv_d, 32);
  hipStream_t st = ctx->stream;
  const u32* idx = (const u32*)d_idx;
  const Fr* deltas = (const Fr*)d_deltas;
  if (d_com) {
    constexpr size_t COM_CHUNK = (size_t)1 << 20;
    ST_TRY(reserve(ctx, ctx->vu_work, std::min(k, COM_CHUNK) * sizeof(G1Jac)));
    G1Jac* terms = (G1Jac*)ctx->vu_work.p;
    for (size_t lo = 0; lo < k; lo += COM_CHUNK) {
      const u32 n = (u32)std::min(COM_CHUNK, k - lo);
      hipLaunchKernelGGL(k_upd_com_terms, dim3(cdiv(n, 64)), dim3(64), 0, st, t.a, t.pw, invd, d, idx + lo, deltas + lo, n, terms);
      hipLaunchKernelGGL(k_upd_com_sum, dim3(1), dim3(64), 0, st, terms, n, (G1Jac*)d_com);
    }
  }
  if (d_proofs) {
    const long long opt = ctx->tune.vec_update_k_pass;
    const size_t kp = opt >= 1 && opt <= (long long)UPD_K_PASS ? (size_t)opt : UPD_K_PASS;
    const size_t hdr_bytes = (sizeof(UpdHdr) + 255) & ~(size_t)255;
    ST_TRY(reserve(ctx, ctx->vu_pass, hdr_bytes + (size_t)UPD_K_PASS * UPD_ROWS * UPD_ROW_WORDS * 4));
    UpdHdr* hdr = (UpdHdr*)ctx->vu_pass.p;
    u32* wtab = (u32*)((char*)ctx->vu_pass.p + hdr_bytes);
    for (size_t lo = 0; lo < k; lo += kp) {
      const u32 cnt = (u32)std::min(kp, k - lo);
      hipLaunchKernelGGL(k_upd_prep, dim3(cnt), dim3(64), 0, st, t.a, t.pw, invd, d, idx + lo, deltas + lo, cnt, hdr, wtab);
      upd_ladder_launches(ctx, d, [&](uint4* tab, u32 first, u32 lanes) {
        if (tab) hipLaunchKernelGGL(k_upd_proofs<true>, dim3(cdiv(lanes, 64)), dim3(64), 0, st, t.a, t.u, t.e, t.pw, (const UpdHdr*)hdr, (const u32*)wtab, cnt, d, (G1Aff*)d_proofs, tab, first);
        else hipLaunchKernelGGL(k_upd_proofs<false>, dim3(cdiv(lanes, 64)), dim3(64), 0, st, t.a, t.u, t.e, t.pw, (const UpdHdr*)hdr, (const u32*)wtab, cnt, d, (G1Aff*)d_proofs, tab, first);
      });
    }
  }
  return launch_check(ctx, "vec_update");
}

}  // namespace keaki_internal
