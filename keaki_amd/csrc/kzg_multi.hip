// KZG set openings: ONE proof for the k points S = {z_0 .. z_(k-1)} of a polynomial p with n coefficients.
//
//   Z(x) = prod (x - z_j)       I(x) = the interpolant of (z_j, p(z_j)), deg < k       pi_S = [((p - I) / Z)(tau)]_1
//
// For distinct points, with the weights c_j = 1 / Z'(z_j) = 1 / prod_(t != j) (z_j - z_t), partial fractions of 1 / Z give
//   (p - I) / Z  =  sum_j c_j (p - p(z_j)) / (x - z_j)
// and every term on the right is the single-point quotient of `open` (fft_g1.hip: Q_i = a_i + z Q_(i+1), quotient coefficient q_(i-1) = Q_i,
// Q_0 = p(z)). tests/kzg_set_model.py is this identity over Z_r, checked against schoolbook long division.
//
// k_mq_*: the blockwise recurrence of fft_g1.hip (up / top / down over blocks of MQ_L coefficients) for a PASS of K points side by side. MQ_L is this
// file's own constant: the results are exact in Fr whatever the block length, nothing depends on it agreeing with fft_g1.hip's HORNER_L.
//   up     a lane reads the 32 coefficients of its block ONCE and runs K Horner chains on them (level 0); the levels above carry K block values
//          per block, one array per point
//   down   a lane re-runs its block from the K carries of the level above; at level 0 it writes out[i - 1] (+)= sum_j c_j Q^(j)_i and, for
//          i = 0, the K values p(z_j) = Q^(j)_0, which fall out for free
// Per coefficient and point: one product up, one down, one by c_j in the weighted sum. A set of k points runs ceil(k / MQ_K) passes; the first
// pass writes the quotient, the later ones add to it (one lane owns an output word: no atomics). A last pass of r < MQ_K points runs the
// instantiation for the next power of two, padded with z = 0, c = 0.
// MQ_K = 8, from the register allocation (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this file): at K = 8 the level-0 up pass takes
// 111 VGPRs and the level-0 down pass 127 (8 carries = 64 of them; the 8 multipliers and 8 weights are wave-uniform and come through SGPRs, 62 of
// which the down pass parks in VGPR lanes), no scratch memory: four waves per SIMD. At K = 4 they take 82 and 94 (five waves each), so
// K = 16 would leave two waves at best. The K-wide arrays are indexed through mq_each (compile-time indices): with plain `#pragma unroll` loops
// the K = 8 instantiations kept the carries in scratch memory (272 bytes per lane).
//
// k_set_polys: Z, the weights and (optionally) I for k <= KEAKI_SET_MAX points, one workgroup, O(k^2) Fr products:
//   Z      thread i owns coefficient i; step j multiplies by (x - z_j): new[i] = old[i - 1] - z_j old[i] (neighbour through LDS)
//   c_j    thread j: the product of its k - 1 differences, then one Fermat inversion
//   I      = sum_j (y_j c_j) Z / (x - z_j). Thread j runs the synthetic division of Z by (x - z_j) from the top, started j steps late, so
//          that in every step the threads add into DIFFERENT coefficients of I (LDS): 2k - 1 steps, no reduction.
// A repeated point makes a difference zero: its weight comes out 0 (Fermat: 0 -> 0) and every result that uses it is meaningless. Distinct
// points are the caller's contract; the kernel does not look.
#include <type_traits>
#include "internal.h"
#include "bn254_curve.hip.h"
#include "kzg_fr.hip.h"

namespace bn254 {

constexpr u32 MQ_L = 32;                 // block length (a chain of 2 x 32 dependent steps per lane and level)
constexpr u32 MQ_K = 8;                  // points per pass
constexpr u32 MQ_LEVELS = 8;

// f(0), f(1), .. f(K - 1) with a compile-time index: the K-wide register arrays below are only ever indexed by constants
template <int K, class F>
KDEV void mq_each(F&& f) {
  if constexpr (K > 0) {
    mq_each<K - 1>(f);
    f(std::integral_constant<int, K - 1>{});
  }
}
KDEV Fr mq_mul(const Fr& a, const Fr& b) { return fp_mul<FrParams>(a, b); }
KDEV Fr mq_add(const Fr& a, const Fr& b) { return fp_add<FrParams>(a, b); }

// The wave-uniform data of a pass: w[lev * K + j] = z_j^(MQ_L^lev), cw[j] = c_j; entries j >= kk are zero (padding).
template <int K>
static __global__ void __launch_bounds__(64) k_mq_prepare(const Fr* __restrict__ z, const Fr* __restrict__ c, u32 kk, u32 levels, Fr* __restrict__ w,
                                                          Fr* __restrict__ cw) {
  const u32 j = threadIdx.x;
  if (blockIdx.x || j >= (u32)K) return;
  Fr x = j < kk ? z[j] : fp_zero<FrParams>();
  cw[j] = j < kk ? c[j] : fp_zero<FrParams>();
#pragma unroll 1
  for (u32 lev = 0; lev < levels; lev++) {
    w[lev * K + j] = x;
    for (u32 s = 1; s < MQ_L; s <<= 1) x = mq_mul(x, x);
  }
}
// H[j * out_stride + b] = sum_(t < L) a_j[b L + t] w_j^t. SHARED (level 0): every point reads the same array a; else a_j = a + j * in_stride.
template <int K, bool SHARED>
static __global__ void __launch_bounds__(64) k_mq_up(const Fr* __restrict__ a, size_t in_stride, u32 m, const Fr* __restrict__ wp, Fr* __restrict__ H,
                                                     size_t out_stride) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lo = b * MQ_L;
  if (b >= (m + MQ_L - 1) / MQ_L) return;
  const u32 hi = min(m, lo + MQ_L);
  if constexpr (SHARED) {
    Fr h[K];
    const Fr top = a[hi - 1];
    mq_each<K>([&](auto j) { h[j] = top; });
#pragma unroll 1
    for (u32 t = hi - 1; t-- > lo;) {
      const Fr cf = a[t];
      mq_each<K>([&](auto j) { h[j] = mq_add(mq_mul(h[j], wp[j]), cf); });
    }
    mq_each<K>([&](auto j) { H[j * out_stride + b] = h[j]; });
  } else {
#pragma unroll 1
    for (int j = 0; j < K; j++) {
      const Fr* aj = a + j * in_stride;
      const Fr w = wp[j];
      Fr h = aj[hi - 1];
#pragma unroll 1
      for (u32 t = hi - 1; t-- > lo;) h = mq_add(mq_mul(h, w), aj[t]);
      H[j * out_stride + b] = h;
    }
  }
}
// levels >= 1: Q_j[t] = suffix value at position t of level array a_j; q_up (null at the top level): the suffix values of the level above
template <int K>
static __global__ void __launch_bounds__(64) k_mq_down(const Fr* __restrict__ a, size_t stride, u32 m, const Fr* __restrict__ wp, const Fr* __restrict__ q_up,
                                                       size_t up_stride, u32 nblocks, Fr* __restrict__ Q) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lo = b * MQ_L;
  if (b >= nblocks) return;
  const u32 hi = min(m, lo + MQ_L);
#pragma unroll 1
  for (int j = 0; j < K; j++) {
    const Fr* aj = a + j * stride;
    Fr* qj = Q + j * stride;
    const Fr w = wp[j];
    Fr carry = (q_up && b + 1 < nblocks) ? q_up[j * up_stride + b + 1] : fp_zero<FrParams>();
#pragma unroll 1
    for (u32 t = hi; t-- > lo;) {
      carry = mq_add(mq_mul(carry, w), aj[t]);
      qj[t] = carry;
    }
  }
}
// level 0: out[t - 1] (+)= sum_j cw_j Q^(j)_t for t >= 1; values[j] = Q^(j)_0 for j < kk
template <int K>
static __global__ void __launch_bounds__(64) k_mq_down0(const Fr* __restrict__ a, u32 m, const Fr* __restrict__ wp, const Fr* __restrict__ cw,
                                                        const Fr* __restrict__ q_up, size_t up_stride, u32 nblocks, Fr* __restrict__ out, u32 accumulate,
                                                        Fr* __restrict__ values, u32 kk) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lo = b * MQ_L;
  if (b >= nblocks) return;
  const u32 hi = min(m, lo + MQ_L);
  Fr carry[K];
  mq_each<K>([&](auto j) { carry[j] = (q_up && b + 1 < nblocks) ? q_up[j * up_stride + b + 1] : fp_zero<FrParams>(); });
#pragma unroll 1
  for (u32 t = hi; t-- > lo;) {
    const Fr cf = a[t];
    mq_each<K>([&](auto j) { carry[j] = mq_add(mq_mul(carry[j], wp[j]), cf); });
    if (t >= 1) {
      Fr acc = mq_mul(carry[0], cw[0]);
      mq_each<K - 1>([&](auto j) { acc = mq_add(acc, mq_mul(carry[j + 1], cw[j + 1])); });
      out[t - 1] = accumulate ? mq_add(out[t - 1], acc) : acc;
    } else {
      mq_each<K>([&](auto j) { if ((u32)j < kk) values[j] = carry[j]; });
    }
  }
}

// zc: k + 1 coefficients of Z (may be null when ic is null) | wts: k weights | ic: k coefficients of I (null: no values given).
// One workgroup of at least k threads (a multiple of 64); zc is read back by other threads of the block: no __restrict__ on it.
static __global__ void __launch_bounds__(1024) k_set_polys(const Fr* __restrict__ z, const Fr* __restrict__ y, u32 k, Fr* zc, Fr* __restrict__ wts,
                                                           Fr* __restrict__ ic) {
  __shared__ Fr sh[KEAKI_SET_MAX];
  const u32 i = threadIdx.x;
  const bool live = i < k;
  // Z: the running product, monic of degree j before step j (thread j holds the leading 1 while j < k)
  Fr cur = i == 0 ? fp_one<FrParams>() : fp_zero<FrParams>();
#pragma unroll 1
  for (u32 j = 0; j < k; j++) {
    const Fr zj = z[j];
    if (live) sh[i] = cur;
    __syncthreads();
    if (live) {
      const Fr prev = i ? sh[i - 1] : fp_zero<FrParams>();
      cur = fp_sub<FrParams>(prev, mq_mul(zj, cur));
    }
    __syncthreads();
  }
  if (zc) {
    if (live) zc[i] = cur;
    if (i == 0) zc[k] = fp_one<FrParams>();
  }
  // the weights
  Fr zi = fp_zero<FrParams>(), c = zi;
  if (live) {
    zi = z[i];
    Fr prod = fp_one<FrParams>();
#pragma unroll 1
    for (u32 t = 0; t < k; t++)
      if (t != i) prod = mq_mul(prod, fp_sub<FrParams>(zi, z[t]));
    c = fr_inv(prod);
    wts[i] = c;
  }
  if (!ic) return;                       // uniform: no barrier below is skipped by a part of the block
  // I: thread i is at coefficient idx = k - 1 - (step - i) of its quotient Z / (x - z_i) in step `step`
  const Fr s = live ? mq_mul(y[i], c) : fp_zero<FrParams>();
  Fr q = fp_one<FrParams>();
  if (live) sh[i] = fp_zero<FrParams>();
  __syncthreads();                       // also makes zc visible to the block
#pragma unroll 1
  for (u32 step = 0; step + 1 < 2 * k; step++) {
    if (live && step >= i && step - i < k) {
      const u32 idx = k - 1 - (step - i);
      if (step > i) q = mq_add(zc[idx + 1], mq_mul(zi, q));
      sh[idx] = mq_add(sh[idx], mq_mul(s, q));
    }
    __syncthreads();
  }
  if (live) ic[i] = sh[i];
}

// verify_multi: out_a = C - I1 (affine), out_z = Z2 (affine) from the two MSM results
static __global__ void __launch_bounds__(64) k_set_pair_points(const G1Aff* __restrict__ com, const G1Jac* __restrict__ i1, const G2Jac* __restrict__ z2,
                                                               G1Aff* __restrict__ out_a, G2Aff* __restrict__ out_z) {
  if (blockIdx.x) return;
  if (threadIdx.x == 0) {
    const G1Jac ni = {i1->x, -i1->y, i1->z};
    *out_a = jac_to_aff(jac_add_mixed(ni, *com));
  } else if (threadIdx.x == 1) {
    *out_z = jac_to_aff(*z2);
  }
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

keaki_status set_polys_run(keaki_hip_ctx* ctx, const void* d_points, const void* d_values, size_t k, void* d_zc, void* d_weights, void* d_ic) {
  if (k == 0 || k > KEAKI_SET_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_set_polys: k = %zu must be in 1 .. %d", k, (int)KEAKI_SET_MAX);
  if (d_ic && (!d_values || !d_zc)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_set_polys: the interpolant needs the values and room for Z");
  hipLaunchKernelGGL(k_set_polys, dim3(1), dim3(cdiv(k, 64) * 64), 0, ctx->stream, (const Fr*)d_points, (const Fr*)d_values, (u32)k, (Fr*)d_zc, (Fr*)d_weights,
                     (Fr*)d_ic);
  return launch_check(ctx, "set_polys");
}

// work of one pass: [w: MQ_LEVELS x MQ_K | cw: MQ_K | level arrays a^1.., then Q^1..: MQ_K rows each]
size_t multi_quotient_work_bytes(size_t n) { return (MQ_LEVELS * MQ_K + MQ_K + 2 * MQ_K * (n / (MQ_L - 1) + 16)) * sizeof(Fr); }

namespace {
template <int K>
keaki_status multi_quotient_pass(keaki_hip_ctx* ctx, const Fr* c, size_t n, const Fr* z, const Fr* wts, u32 kk, Fr* out, bool accumulate, Fr* values, Fr* work) {
  hipStream_t st = ctx->stream;
  u32 m[MQ_LEVELS];
  u32 levels = 0;
  for (size_t cur = n;; cur = (cur + MQ_L - 1) / MQ_L) { m[levels++] = (u32)cur; if (cur <= MQ_L || levels == MQ_LEVELS) break; }
  Fr* w = work;
  Fr* cw = w + MQ_LEVELS * K;
  Fr* p = work + MQ_LEVELS * MQ_K + MQ_K;
  Fr *a[MQ_LEVELS], *Q[MQ_LEVELS];
  a[0] = nullptr; Q[0] = nullptr;
  for (u32 l = 1; l < levels; l++) { a[l] = p; p += (size_t)K * m[l]; }
  for (u32 l = 1; l < levels; l++) { Q[l] = p; p += (size_t)K * m[l]; }
  hipLaunchKernelGGL(k_mq_prepare<K>, dim3(1), dim3(64), 0, st, z, wts, kk, levels, w, cw);
  for (u32 l = 0; l + 1 < levels; l++) {
    if (l == 0) hipLaunchKernelGGL((k_mq_up<K, true>), dim3(cdiv(m[1], 64)), dim3(64), 0, st, c, (size_t)0, m[0], (const Fr*)w, a[1], (size_t)m[1]);
    else hipLaunchKernelGGL((k_mq_up<K, false>), dim3(cdiv(m[l + 1], 64)), dim3(64), 0, st, (const Fr*)a[l], (size_t)m[l], m[l], (const Fr*)(w + l * K), a[l + 1], (size_t)m[l + 1]);
  }
  for (u32 l = levels; l-- > 0;) {
    const Fr* q_up = (l + 1 < levels) ? Q[l + 1] : nullptr;
    const size_t up_stride = (l + 1 < levels) ? m[l + 1] : 0;
    const u32 nblocks = cdiv(m[l], MQ_L);
    if (l == 0)
      hipLaunchKernelGGL(k_mq_down0<K>, dim3(cdiv(nblocks, 64)), dim3(64), 0, st, c, m[0], (const Fr*)w, (const Fr*)cw, q_up, up_stride, nblocks, out, accumulate ? 1u : 0u,
                         values, kk);
    else
      hipLaunchKernelGGL(k_mq_down<K>, dim3(cdiv(nblocks, 64)), dim3(64), 0, st, (const Fr*)a[l], (size_t)m[l], m[l], (const Fr*)(w + l * K), q_up, up_stride, nblocks, Q[l]);
  }
  return launch_check(ctx, "multi_quotient");
}
}  // namespace

// d_c: n >= 1 coefficients. d_q: the n - 1 coefficients of sum_j c_j (p - p(z_j)) / (x - z_j) (nothing written for n == 1). d_values: k Fr, p(z_j).
// d_points, d_weights: k Fr each (set_polys_run). d_work: multi_quotient_work_bytes(n).
keaki_status multi_quotient_run(keaki_hip_ctx* ctx, const void* d_c, size_t n, const void* d_points, const void* d_weights, size_t k, void* d_q, void* d_values,
                                void* d_work) {
  if (n == 0 || n >= ((size_t)1 << 32) || k == 0) return fail(ctx, KEAKI_ERR_BAD_ARG, "multi_quotient: n = %zu, k = %zu out of range", n, k);
  const Fr *c = (const Fr*)d_c, *z = (const Fr*)d_points, *wt = (const Fr*)d_weights;
  Fr *out = (Fr*)d_q, *val = (Fr*)d_values, *work = (Fr*)d_work;
  for (size_t j0 = 0; j0 < k; j0 += MQ_K) {
    const u32 kk = (u32)std::min<size_t>(MQ_K, k - j0);
    const bool acc = j0 != 0;
    if (kk == 1) ST_TRY(multi_quotient_pass<1>(ctx, c, n, z + j0, wt + j0, kk, out, acc, val + j0, work));
    else if (kk == 2) ST_TRY(multi_quotient_pass<2>(ctx, c, n, z + j0, wt + j0, kk, out, acc, val + j0, work));
    else if (kk <= 4) ST_TRY(multi_quotient_pass<4>(ctx, c, n, z + j0, wt + j0, kk, out, acc, val + j0, work));
    else ST_TRY(multi_quotient_pass<8>(ctx, c, n, z + j0, wt + j0, kk, out, acc, val + j0, work));
  }
  return KEAKI_OK;
}

keaki_status set_pair_points_run(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_i1_jac, const void* d_z2_jac, void* d_out_a_aff, void* d_out_z_aff) {
  hipLaunchKernelGGL(k_set_pair_points, dim3(1), dim3(64), 0, ctx->stream, (const G1Aff*)d_com_aff, (const G1Jac*)d_i1_jac, (const G2Jac*)d_z2_jac,
                     (G1Aff*)d_out_a_aff, (G2Aff*)d_out_z_aff);
  return launch_check(ctx, "set_pair_points");
}

}  // namespace keaki_internal
