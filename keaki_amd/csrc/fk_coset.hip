// FK23 coset openings ("multi-reveal"): all r = d / l set proofs of a polynomial p (d = 2^log2d coefficients) for the l-point cosets of the
// size-d evaluation domain in one pass. Coset i < r is the index set {i + t r : t < l}; its points are the l solutions of x^l = c_i,
// c_i = omega_r^i, so Z_i(x) = x^l - c_i and the proof is pi_i = [floor(p / (x^l - c_i))(tau)]_1 -- what keaki_hip_kzg_open_multi returns for
// those l points.
//
// Dividing by x^l - c gives pi_i = sum_{t = 1..r} c_i^(t-1) h_t with h_t = sum_{m >= t l} f_m [tau^(m - t l)]_1; with m - t l = v l + j, j < l:
//   h_t = sum_{j < l} sum_{u >= t} f_(u l + j) srs[(u - t) l + j]
// i.e. for every residue j the Toeplitz product of open_fk (fft_g1.hip) at size r over the rows S(j)_v = srs[v l + j], F(j)_u = f_(u l + j):
//   hat_s_j = DFT_2r(S(j) reversed, then r identities)        k_fkc_load + g1_dif_run per row; cached per (SRS, d, l): position q holds index brev(q)
//   hat_a_j = DFT_2r(r zeros, then F(j)) / 2r                 k_fkc_pad (scale and bit reversal folded in) + k_fkc_fr_stage, all l rows per launch
//   hat_h[q] = sum_{j < l} hat_a_j[brev(q)] hat_s_j[q]        k_fkc_pointwise: THE HOT KERNEL, below
//   h = first r of DFT_2r^-1(hat_h)                           k_fkc_gather (sums the S partial sums, un-permutes) + g1_dif_run + k_fkc_take
//   (pi_0 .. pi_(r-1)) = DFT_r(h)                             g1_dif_run + k_fkc_finish (affine, natural order)
// l = 1 is open_fk itself; r = 1 gives the identity (deg p < d = l) and runs nothing. tests/fk_coset_model.py is this file over Z_r.
//
// k_fkc_pointwise: lane (s, q) owns the terms [s l / S, (s + 1) l / S) of position q and runs them in groups of G. A group is ONE Straus chain:
// every term's scalar is split with GLV into two halves of 33 signed 4-bit windows (jac29.hip.h: glv_decompose, glv_fixed_digits, as
// jac_scalar_mul_gtab_u29_j), every term gets its own window table {1..8} P in the lane's slice of the table workspace (G x 1 KB, the layout of
// J29GlobTable: an entry is one 128-byte line), and ONE running point takes 33 x (4 doublings + 2 G mixed additions): 129 doublings per group
// instead of per term. The G tables are built independently (each effective-affine on its own curve E_(z_g), j29_build_table) and then brought to
// the ONE curve E_Z, Z = prod z_g: table g is rescaled by s_g = prod_(h != g) z_h (x s^2, beta x s^2, y s^3: 24 products per table, from prefix
// and suffix products, no inversion), the result's Z is multiplied by Z. The other way this tree knows (j29_build_pair: build table B on the
// curve of table A, rescale A) rescales the earlier tables once per later table: G (G - 1) / 2 table passes instead of G. The digits wait in
// LDS (14 words per term, lane-strided: no bank conflict, no scratch), the z_g in the five spare words of the table lines. Identity bases
// and zero scalars get no table and all-zero digits. Groups, and the S lanes of a position, meet in jac_add.
// Cache: Jacobian points (192 B x d), the form g1_dif_run leaves; the table build reads any Z.
#include "jac29.hip.h"
#include "internal.h"
#include "fk_coset_plan.h"

namespace bn254 {

constexpr u32 FKC_G_MAX = keaki_internal::FKC_G;
constexpr u32 FKC_DIG_WORDS = 14;            // per term: [half 1: 5 words of magnitudes, 2 of signs | half 2: the same]
constexpr u32 FKC_TAB_WORDS = GTAB_UINT4_PER_LANE * 4;

KDEV u32 fkc_brev(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }

// row j of the transform's input: out[j 2r + k] = srs[(r - 1 - k) l + j] (k < r), the identity (k >= r)
static __global__ void __launch_bounds__(256) k_fkc_load(const G1Aff* __restrict__ srs, u32 log2r, u32 log2l, G1Jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 r = 1u << log2r, n2 = 2 * r;
  if (i >= ((size_t)n2 << log2l)) return;
  const u32 j = (u32)(i >> (log2r + 1)), k = (u32)i & (n2 - 1);
  out[i] = k < r ? jac_from_aff(srs[((size_t)(r - 1 - k) << log2l) + j]) : jac_inf<Fq>();
}
// the padded rows of the scalar transforms, scaled and already in bit-reversed order: a[j 2r + brev(k)] = scale * (k < r ? 0 : p[(k - r) l + j])
static __global__ void __launch_bounds__(256) k_fkc_pad(const Fr* __restrict__ p, u32 log2r, u32 log2l, Fr scale, Fr* __restrict__ a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 r = 1u << log2r, n2 = 2 * r;
  if (i >= ((size_t)n2 << log2l)) return;
  const u32 j = (u32)(i >> (log2r + 1)), k = (u32)i & (n2 - 1);
  a[((size_t)j << (log2r + 1)) + fkc_brev(k, log2r + 1)] = k < r ? fp_zero<FrParams>() : fp_mul<FrParams>(p[((size_t)(k - r) << log2l) + j], scale);
}
// one radix-2 stage (span len) of ALL rows: butterfly b of row b / r. tw[k] = omega_2r^k, k < r
static __global__ void __launch_bounds__(256) k_fkc_fr_stage(Fr* __restrict__ a, const Fr* __restrict__ tw, u32 log2r, u32 log2l, u32 len) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 r = 1u << log2r, n2 = 2 * r;
  if (i >= ((size_t)r << log2l)) return;
  const u32 b = (u32)i & (r - 1), half = len >> 1;
  Fr* row = a + ((i >> log2r) << (log2r + 1));
  const u32 j = b % half, i0 = (b / half) * len + j, i1 = i0 + half;
  const Fr u = row[i0], v = fp_mul<FrParams>(row[i1], tw[(size_t)j * (n2 / len)]);
  row[i0] = fp_add<FrParams>(u, v);
  row[i1] = fp_sub<FrParams>(u, v);
}
static __global__ void __launch_bounds__(256) k_fkc_stride2(const Fr* __restrict__ in, u32 n_out, Fr* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_out) out[i] = in[2 * (size_t)i];
}

// the spare words [27..31] of two neighbouring table lines hold one U29: slot 0 (lines 0, 1) = z_g, slot 1 (lines 2, 3) = prod_(h > g) z_h
KDEV void fkc_st_spare(u32* __restrict__ tb, int slot, const U29& v) {
  u32 *e0 = tb + 64 * slot + 27, *e1 = e0 + 32;
#pragma unroll
  for (int i = 0; i < 5; i++) e0[i] = v.l[i];
#pragma unroll
  for (int i = 0; i < 4; i++) e1[i] = v.l[5 + i];
}
KDEV U29 fkc_ld_spare(const u32* __restrict__ tb, int slot) {
  const u32 *e0 = tb + 64 * slot + 27, *e1 = e0 + 32;
  U29 v;
#pragma unroll
  for (int i = 0; i < 5; i++) v.l[i] = e0[i];
#pragma unroll
  for (int i = 0; i < 4; i++) v.l[5 + i] = e1[i];
  return v;
}

// partial[s 2r + q] = sum_{j in slice s} a[j 2r + brev(q)] hs[j 2r + q]; lane t = s 2r + q of `lanes` = S 2r, this launch covers [first, first + 64 gridDim.x);
// tab: G KB per lane of the launch. G in {1, 2, 4} (1: one ladder per term, no rescaling -- the A/B form of option fk_coset_group)
static __global__ void __launch_bounds__(64) k_fkc_pointwise(const G1Jac* __restrict__ hs, const Fr* __restrict__ a, u32 L2, u32 per_lane, u32 G, u32 groups,
                                                             G1Jac* __restrict__ partial, uint4* __restrict__ tab, u32 first, u32 lanes) {
  __shared__ u32 dg[FKC_G_MAX * FKC_DIG_WORDS * 64];
  const u32 lane = threadIdx.x;
  const u32 t = first + blockIdx.x * 64 + lane;
  if (t >= lanes) return;
  const u32 n2 = 1u << L2, q = t & (n2 - 1), s = t >> L2, qa = fkc_brev(q, L2);
  u32* const mytab = reinterpret_cast<u32*>(tab) + (size_t)(t - first) * G * FKC_TAB_WORDS;
  const U29 beta = u29_const(GlvParams::BETA29);
  U29 zero;
#pragma unroll
  for (int i = 0; i < 9; i++) zero.l[i] = 0;
  G1Jac total = jac_inf<Fq>();
#pragma unroll 1
  for (u32 grp = 0; grp < groups; grp++) {
    const u32 j0 = s * per_lane + grp * G;
    // 1. digits and window tables, one term after the other
    u32 any = 0;
#pragma unroll 1
    for (u32 g = 0; g < G; g++) {
      const size_t row = (size_t)(j0 + g) << L2;
      const G1Jac p = hs[row + q];
      const Fr sc = a[row + qa];
      u32* const tb32 = mytab + g * FKC_TAB_WORDS;
      u32* const d = dg + g * FKC_DIG_WORDS * 64 + lane;
      U29 zf = u29_one();
      if (!jac_is_inf(p) && !fp_is_zero<FrParams>(sc)) {
        u32 k[8], k1[5], k2[5], dig[5], sg[2];
        bool neg1, neg2;
        fp_from_mont<FrParams>(k, sc);
        glv_decompose(k, k1, neg1, k2, neg2);
        glv_fixed_digits(k1, dig, sg);
#pragma unroll
        for (int i = 0; i < 5; i++) d[i * 64] = dig[i];
        d[5 * 64] = neg1 ? ~sg[0] : sg[0];          // the half's own sign rides on every digit's
        d[6 * 64] = neg1 ? ~sg[1] : sg[1];
        glv_fixed_digits(k2, dig, sg);
#pragma unroll
        for (int i = 0; i < 5; i++) d[(7 + i) * 64] = dig[i];
        d[12 * 64] = neg2 ? ~sg[0] : sg[0];
        d[13 * 64] = neg2 ? ~sg[1] : sg[1];
        J29GlobTable tb;
        tb.base = tb32;
        tb.beta = beta;
        zf = j29_build_table<false>(p, tb);
        asm volatile("" ::: "memory");
        any = 1;
      } else {
#pragma unroll
        for (u32 i = 0; i < FKC_DIG_WORDS; i++) d[i * 64] = 0;
      }
      fkc_st_spare(tb32, 0, zf);
    }
    if (!any) continue;
    // 2. every table onto the curve E_Z, Z = prod z_g
    U29 zall;
    if (G > 1) {
      U29 run = u29_one();
#pragma unroll 1
      for (int g = (int)G - 1; g >= 0; g--) {
        u32* const tb32 = mytab + g * FKC_TAB_WORDS;
        const U29 zf = fkc_ld_spare(tb32, 0);
        fkc_st_spare(tb32, 1, run);
        run = u29_mul(run, zf);
      }
      zall = run;
      U29 pre = u29_one();
#pragma unroll 1
      for (u32 g = 0; g < G; g++) {
        u32* const tb32 = mytab + g * FKC_TAB_WORDS;
        const U29 sg = u29_mul(pre, fkc_ld_spare(tb32, 1));
        pre = u29_mul(pre, fkc_ld_spare(tb32, 0));
        const u32* const d = dg + g * FKC_DIG_WORDS * 64 + lane;
        u32 used = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) used |= d[i * 64] | d[(7 + i) * 64];
        if (!used) continue;                         // no table was built
        const U29 s2 = u29_sqr(sg), s3 = u29_mul(sg, s2);
#pragma unroll 1
        for (int i = 0; i < 8; i++) {
          u32* const e = tb32 + 32 * i;
          const U29 y = ld9(e), x = ld9(e + 9), xb = ld9(e + 18);
          st9(e, u29_mul(y, s3));
          st9(e + 9, u29_mul(x, s2));
          st9(e + 18, u29_mul(xb, s2));
        }
      }
      asm volatile("" ::: "memory");
    } else {
      zall = fkc_ld_spare(mytab, 0);
    }
    // 3. one chain for the group
    J29 acc;
    acc.x = zero; acc.y = zero; acc.z = zero;
    bool empty = true;
#pragma unroll 1
    for (int jw = 32; jw >= 0; jw--) {
      if (!empty) { acc = j29_dbl(acc); acc = j29_dbl(acc); acc = j29_dbl(acc); acc = j29_dbl(acc); }
#pragma unroll 1
      for (u32 th = 0; th < 2 * G; th++) {
        const u32 g = th >> 1, which = th & 1u;
        const u32* const d = dg + (g * FKC_DIG_WORDS + which * 7) * 64 + lane;
        const u32 mag = (d[(jw >> 3) * 64] >> ((jw & 7) * 4)) & 15u;
        if (mag) {
          const bool neg = ((d[(5 + (jw >> 5)) * 64] >> (jw & 31)) & 1u) != 0;
          const u32* const e32 = mytab + g * FKC_TAB_WORDS + (mag - 1u) * 32u;
          const U29 ex = ld9(e32 + (which ? 18 : 9));
          const U29 y = ld9(e32);
          const U29 ey = neg ? u29_sub(zero, y, Q29::K4) : y;
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
    if (empty) continue;
    J29 res;
    res.x = acc.x; res.y = acc.y; res.z = u29_mul(acc.z, zall);
    total = jac_add(total, j29_to_sat(res));
  }
  partial[t] = total;
}
// out[brev(q)] = sum_s partial[s 2r + q]: hat_h in natural order
static __global__ void __launch_bounds__(64) k_fkc_gather(const G1Jac* __restrict__ partial, u32 S, u32 L2, G1Jac* __restrict__ out) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (1u << L2)) return;
  G1Jac acc = partial[q];
  for (u32 s = 1; s < S; s++) acc = jac_add(acc, partial[((size_t)s << L2) + q]);
  out[fkc_brev(q, L2)] = acc;
}
// out[k] = in[brev(k)], k < r: the first r entries of a size-2r transform that g1_dif_run left in bit-reversed positions
static __global__ void __launch_bounds__(256) k_fkc_take(const G1Jac* __restrict__ in, u32 L2, G1Jac* __restrict__ out) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (1u << (L2 - 1))) return;
  out[k] = in[fkc_brev(k, L2)];
}
static __global__ void __launch_bounds__(64) k_fkc_finish(const G1Jac* __restrict__ in, u32 log2r, G1Aff* __restrict__ out) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (1u << log2r)) return;
  out[fkc_brev(q, log2r)] = jac_to_aff(in[q]);
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

// most lanes of one pointwise launch: the table workspace (ctx->fk_tab, shared with the FK23 ladders) holds at most 2^21 KB
constexpr size_t FKC_TAB_KB_MAX = (size_t)1 << 21;

size_t fkc_fr_bytes(uint32_t log2d, uint32_t log2l) {       // tw r | twi r | tw_r r / 2 (+ slack) | hat_a 2d
  const size_t r = (size_t)1 << (log2d - log2l);
  return (2 * r + r / 2 + 2 + ((size_t)2 << log2d)) * sizeof(Fr);
}
size_t fkc_g_bytes(uint32_t log2d, uint32_t log2l, const FkcPlan& plan) {       // partial sums S 2r | hat_h 2r | h r
  const size_t r = (size_t)1 << (log2d - log2l);
  return ((size_t)plan.S * 2 * r + 3 * r) * sizeof(G1Jac);
}
FkcScalars fkc_layout(uint32_t log2d, uint32_t log2l, void* d_fr_work) {
  const size_t r = (size_t)1 << (log2d - log2l);
  Fr* tw = (Fr*)d_fr_work;
  return {tw, tw + r, tw + 2 * r, tw + 2 * r + r / 2 + 2};
}
// the table workspace for `lanes` lanes of G tables each; *lanes_per_launch: what one launch may cover
keaki_status fkc_reserve_tab(keaki_hip_ctx* ctx, size_t lanes, uint32_t G, uint32_t* lanes_per_launch) {
  const size_t kb = std::min(lanes * G, FKC_TAB_KB_MAX);
  ST_TRY(reserve(ctx, ctx->fk_tab, kb * 1024));
  *lanes_per_launch = (uint32_t)(kb / G);
  return KEAKI_OK;
}
// omega_2r^k, omega_2r^-k (k < r) and omega_r^k (k < r / 2) into the layout's tables; r >= 2
keaki_status fkc_tables_run(keaki_hip_ctx* ctx, uint32_t log2r, const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const FkcScalars& s) {
  const uint32_t r = 1u << log2r;
  fr_powers_run(ctx, omega_2r, r, (void*)s.tw);
  fr_powers_run(ctx, omega_2r_inv, r, (void*)s.twi);
  hipLaunchKernelGGL(k_fkc_stride2, dim3(cdiv(r / 2, 256)), dim3(256), 0, ctx->stream, (const Fr*)s.tw, r / 2, (Fr*)s.twr);
  return launch_check(ctx, "fk_coset tables");
}
// the l transforms hat_s_j, row j at d_hat_s + j 2r. d_tw: omega_2r^k, k < r, ready in stream order
keaki_status fkc_hat_s_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2d, uint32_t log2l, const void* d_tw, void* d_hat_s) {
  const uint32_t log2r = log2d - log2l;
  const size_t n2 = (size_t)2 << log2r, l = (size_t)1 << log2l;
  hipLaunchKernelGGL(k_fkc_load, dim3(cdiv(n2 * l, 256)), dim3(256), 0, ctx->stream, (const G1Aff*)d_srs, log2r, log2l, (G1Jac*)d_hat_s);
  for (size_t j = 0; j < l; j++) ST_TRY(g1_dif_run(ctx, (G1Jac*)d_hat_s + j * n2, log2r + 1, d_tw));
  return launch_check(ctx, "fk_coset hat_s");
}
// hat_a from the d coefficients at d_p: l rows of 2r, natural order, divided by 2r
keaki_status fkc_scalars_run(keaki_hip_ctx* ctx, uint32_t log2d, uint32_t log2l, const void* d_p, const uint64_t* inv_2r, const FkcScalars& s) {
  const uint32_t log2r = log2d - log2l;
  const size_t n2 = (size_t)2 << log2r, l = (size_t)1 << log2l;
  Fr sc;
  memcpy(&sc, inv_2r, 32);
  hipLaunchKernelGGL(k_fkc_pad, dim3(cdiv(n2 * l, 256)), dim3(256), 0, ctx->stream, (const Fr*)d_p, log2r, log2l, sc, (Fr*)s.hat_a);
  for (uint32_t len = 2; len <= n2; len <<= 1)
    hipLaunchKernelGGL(k_fkc_fr_stage, dim3(cdiv(n2 / 2 * l, 256)), dim3(256), 0, ctx->stream, (Fr*)s.hat_a, (const Fr*)s.tw, log2r, log2l, len);
  return launch_check(ctx, "fk_coset scalars");
}
// r = d / l >= 2 coset proofs from the cached transforms and hat_a. d_g_work: fkc_g_bytes; the table workspace is reserved (fkc_reserve_tab).
keaki_status fkc_open_run(keaki_hip_ctx* ctx, const void* d_hat_s, uint32_t log2d, uint32_t log2l, const FkcScalars& s, const FkcPlan& plan,
                          uint32_t lanes_per_launch, void* d_g_work, void* d_proofs_aff) {
  const uint32_t log2r = log2d - log2l, L2 = log2r + 1, r = 1u << log2r, n2 = 2 * r, l = 1u << log2l;
  hipStream_t st = ctx->stream;
  G1Jac *partial = (G1Jac*)d_g_work, *hh = partial + (size_t)plan.S * n2, *h = hh + n2;
  const bool timed = ctx->timing && ctx->fk_ev[0];
  if (timed) (void)hipEventRecord(ctx->fk_ev[0], st);
  const size_t lanes = (size_t)plan.S * n2;
  for (size_t first = 0; first < lanes; first += lanes_per_launch) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(lanes_per_launch, lanes - first);
    hipLaunchKernelGGL(k_fkc_pointwise, dim3(cdiv(cnt, 64)), dim3(64), 0, st, (const G1Jac*)d_hat_s, (const Fr*)s.hat_a, L2, l / plan.S, plan.G, plan.groups,
                       partial, (uint4*)ctx->fk_tab.p, (uint32_t)first, (uint32_t)std::min<size_t>(lanes, first + cnt));
  }
  if (timed) (void)hipEventRecord(ctx->fk_ev[1], st);
  hipLaunchKernelGGL(k_fkc_gather, dim3(cdiv(n2, 64)), dim3(64), 0, st, (const G1Jac*)partial, plan.S, L2, hh);
  ST_TRY(g1_dif_run(ctx, hh, L2, s.twi));
  hipLaunchKernelGGL(k_fkc_take, dim3(cdiv(r, 256)), dim3(256), 0, st, (const G1Jac*)hh, L2, h);
  ST_TRY(g1_dif_run(ctx, h, log2r, s.twr));
  if (timed) (void)hipEventRecord(ctx->fk_ev[2], st);
  hipLaunchKernelGGL(k_fkc_finish, dim3(cdiv(r, 64)), dim3(64), 0, st, (const G1Jac*)h, log2r, (G1Aff*)d_proofs_aff);
  if (timed) { (void)hipEventRecord(ctx->fk_ev[3], st); ctx->fk_timing_pending = true; }
  return launch_check(ctx, "open_fk_cosets");
}

}  // namespace keaki_internal
