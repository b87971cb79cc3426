// KZG set pairs (keaki_hip_kzg_set_pairs): the G2 side. For item i (k DISTINCT points with k claimed values) the call returns
//     A_i = C_i - [I_i(tau)]_1        Z2_i = [Z_i(tau)]_2 = [tau^k]_2 + sum_(t < k) Z_(i,t) [tau^t]_2
// the two per-item inputs of the set check e(A_i, g2) == e(proof_i, Z2_i). The Fr side (kzg_sets.hip: k_vs_points, k_vs_weights, k_vs_polys<1 / 2>) leaves, per
// launch chunk, the rows -I_(i,t) (padded to kp, the layout of the coset rows) and Z_(i,t), t < k, 32 B each. A_i is the group side of coset_pairs at
// log2l = log2 kp (kzg_coset_pairs.hip). What lives here:
//   g2_fb_tables_run  the window table T2[j][w][d] = d 2^(wb w) [tau^j]_2 over the first kb G2 points of the SRS, by the two ladders of the fixed-base tables
//                 (ec_batch.hip.h: k_fb_window_bases, k_fb_table_entries), base-major; wb from set_rows_plan.h. The G2 handle keeps it.
//   k_sp_rows_g2  all rows share the bases [tau^t]_2, so a row costs k x windows additions and no doublings. A lane owns one (item, slice of the kp base slots):
//                 it walks the signed wb-bit digits of each of its scalars exactly as fb_accumulate_g2_u29 does (carry into the next digit included) and adds
//                 the table entries to an accumulator in the lazy 29-bit XYZZ form (xyzz29_g2.hip.h). x29g2_add_mixed is a complete addition: equal
//                 operands double, opposite ones give the identity and the walk goes on, an identity entry (an SRS point (0,0)) is skipped. The S slices of an
//                 item sit in neighbouring lanes of one wave and meet in log2 S rounds of cross-lane exchange (73 words a round) with the general addition
//                 x29g2_add, entered through the canonical form (the mixed chain allows its accumulator wider bounds than the general addition is modelled
//                 for); slice 0 adds [tau^k]_2 (Z is monic) and stores the sum in XYZZ.
//   k_sp_affine_g2  XYZZ -> affine with (0,0) for the identity, SP_INV = 4 items per lane under ONE Fq2 inversion (Montgomery's trick over the zzz).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this file; no atomics):
//   k_sp_rows_g2    256 VGPRs + 18 AGPRs, no scratch memory, 384 B LDS (the compiler's, for the cross-lane moves), one wave per SIMD
//   k_sp_affine_g2  204 VGPRs, 96 B of scratch memory per lane (the call frame of the outlined Fq2 product, as in every G2 kernel of ec_batch.hip.h), no LDS
#define KEAKI_FQ2_OUTLINE 1
#include "ec_batch.hip.h"
#include "internal.h"
namespace keaki_internal {
using namespace bn254;

constexpr u32 SP_INV = 4;

KDEV L2 sp_shfl_xor(const L2& a, u32 mask) {
  L2 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.a.l[i] = (u32)__shfl_xor((int)a.a.l[i], (int)mask, 64);
    r.b.l[i] = (u32)__shfl_xor((int)a.b.l[i], (int)mask, 64);
  }
  return r;
}
KDEV X29G2 sp_shfl_xor(const X29G2& a, u32 mask) {
  X29G2 r;
  r.x = sp_shfl_xor(a.x, mask); r.y = sp_shfl_xor(a.y, mask); r.zz = sp_shfl_xor(a.zz, mask); r.zzz = sp_shfl_xor(a.zzz, mask);
  r.empty = __shfl_xor((int)a.empty, (int)mask, 64) != 0;
  return r;
}

// lane = item * S + slice over the m items of a chunk; S = 2^log2S <= min(kp, 64) divides the wave, so an item never straddles two waves. Lanes past
// m * S redo the last item (the exchange needs every lane of a wave) and store nothing. Base slots at or above k hold nothing.
static __global__ void __launch_bounds__(64) k_sp_rows_g2(const G2Aff* __restrict__ table, FbShape g, const u32* __restrict__ rows, u32 k, u32 log2kp, u32 log2S,
                                                          const G2Aff* __restrict__ tau_k, u32 m, G2Xyzz* __restrict__ out) {
  const u32 lane = blockIdx.x * 64u + threadIdx.x;
  const u32 item = lane >> log2S, slice = lane & ((1u << log2S) - 1u);
  const bool live = item < m;
  const u32 it = live ? item : m - 1u;
  const u32 per = 1u << (log2kp - log2S), half = 1u << (g.wb - 1);
  const size_t per_base = (size_t)g.windows * g.entries;
  const u32 j_end = min((slice + 1u) * per, k);
  X29G2 acc = x29g2_inf();
#pragma unroll 1
  for (u32 j = slice * per; j < j_end; j++) {
    const uint4* src = reinterpret_cast<const uint4*>(rows + ((size_t)it * k + j) * 8u);
    const uint4 lo = src[0], hi = src[1];
    u32 v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const G2Aff* tab = table + (size_t)j * per_base;
    u32 carry = 0;
#pragma unroll 1
    for (u32 w = 0; w < g.windows; w++) {
      u32 d = (v[0] & (2u * half - 1u)) + carry;
#pragma unroll
      for (int t = 0; t < 7; t++) v[t] = (v[t] >> g.wb) | (v[t + 1] << (32u - g.wb));
      v[7] >>= g.wb;
      const bool neg = d > half;                       // d - 2^wb and a carry (2^wb itself: digit 0, carry 1)
      carry = neg ? 1u : 0u;
      if (neg) d = 2u * half - d;
      if (d) x29g2_add_mixed(acc, aff_cneg(tab[(size_t)w * g.entries + d], neg));
    }
  }
  if (log2S) {
    acc = x29g2_load(x29g2_store(acc));                // the general addition's working form
#pragma unroll 1
    for (u32 step = 1; step < (1u << log2S); step <<= 1) acc = x29g2_add(acc, sp_shfl_xor(acc, step));   // every lane adds; slice 0 holds the item's sum
  }
  if (!live || slice) return;
  x29g2_add_mixed(acc, *tau_k);
  out[item] = x29g2_store(acc);
}

static __global__ void __launch_bounds__(64) k_sp_affine_g2(const G2Xyzz* __restrict__ in, u32 m, G2Aff* __restrict__ out) {
  const u32 k0 = (blockIdx.x * 64u + threadIdx.x) * SP_INV;
  if (k0 >= m) return;
  Fq2 pre[SP_INV];                                   // pre[i] = zzz_k0 .. zzz_(k0 + i), an identity or a slot past m counting as one
  Fq2 run = f_one<Fq2>();
#pragma unroll
  for (u32 i = 0; i < SP_INV; i++) {
    if (k0 + i < m) {
      const Fq2 zzz = in[k0 + i].zzz;
      if (!f_is_zero(zzz)) run = run * zzz;
    }
    pre[i] = run;
  }
  Fq2 inv = f_inv(run);
#pragma unroll
  for (u32 t = 0; t < SP_INV; t++) {
    const u32 i = SP_INV - 1u - t;                   // a compile-time index after unrolling: pre[] stays in registers
    if (k0 + i < m) {
      const G2Xyzz p = in[k0 + i];
      G2Aff r = aff_inf<Fq2>();
      if (!f_is_zero(p.zz)) {
        const Fq2 izzz = i ? inv * pre[i ? i - 1u : 0u] : inv;
        inv = inv * p.zzz;
        const Fq2 izz = f_sqr(izzz) * f_sqr(p.zz);   // zz^-1 = zzz^-2 zz^2 (zz^3 = zzz^2)
        r = {p.x * izz, p.y * izzz};
      }
      out[k0 + i] = r;
    }
  }
}

// table[(b * windows + j) * entries + d] = d 2^(wb j) * bases[b], b < n_bases: g1_fb_tables_run (ec_batch_g1.hip) on G2
keaki_status g2_fb_tables_run(keaki_hip_ctx* ctx, const void* d_bases, uint32_t n_bases, void* d_table, uint32_t wb) {
  const FbShape g = fb_shape(wb);
  const u32 rows = n_bases * g.windows;
  if (n_bases == 0 || (size_t)rows * g.entries >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g2_fb_tables: %u bases at %u bits out of range", n_bases, wb);
  ST_TRY(reserve(ctx, ctx->fb_bases, (size_t)rows * sizeof(G2Aff)));
  hipLaunchKernelGGL((k_fb_window_bases<Fq2>), dim3(cdiv(rows, 64)), dim3(64), 0, ctx->stream, (const G2Aff*)d_bases, g, (G2Aff*)ctx->fb_bases.p, n_bases);
  const FbShape all = {g.wb, rows, g.entries};
  hipLaunchKernelGGL((k_fb_table_entries<Fq2>), dim3(cdiv((size_t)rows * g.entries, 64)), dim3(64), 0, ctx->stream, (const G2Aff*)ctx->fb_bases.p, all,
                     (G2Aff*)d_table);
  return launch_check(ctx, "g2_fb_tables");
}

keaki_status set_rows_g2_run(keaki_hip_ctx* ctx, const void* d_table, uint32_t wb, const void* d_rows_z, size_t k, uint32_t S, const void* d_tau_k_g2, size_t m,
                             void* d_xyzz) {
  u32 log2S = 0, log2kp = 0;
  while ((1u << log2S) < S) log2S++;
  while (((size_t)1 << log2kp) < k) log2kp++;
  if (m == 0 || k == 0 || k > KEAKI_VERIFY_SETS_K_MAX || (1u << log2S) != S || log2S > 6 || log2S > log2kp || (m << log2kp) >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_set_pairs: a chunk of %zu items of %zu points in %u slices out of range on the device side", m, k, S);
  hipLaunchKernelGGL(k_sp_rows_g2, dim3(cdiv(m << log2S, 64)), dim3(64), 0, ctx->stream, (const G2Aff*)d_table, fb_shape(wb), (const u32*)d_rows_z, (u32)k, log2kp,
                     log2S, (const G2Aff*)d_tau_k_g2, (u32)m, (G2Xyzz*)d_xyzz);
  return launch_check(ctx, "set_rows_g2");
}

keaki_status set_rows_affine_g2_run(keaki_hip_ctx* ctx, const void* d_xyzz, size_t m, void* d_out_aff) {
  if (m == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_sp_affine_g2, dim3(cdiv(cdiv(m, SP_INV), 64)), dim3(64), 0, ctx->stream, (const G2Xyzz*)d_xyzz, (u32)m, (G2Aff*)d_out_aff);
  return launch_check(ctx, "set_rows_affine_g2");
}

}  // namespace keaki_internal
