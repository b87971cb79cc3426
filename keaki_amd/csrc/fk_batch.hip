// FK23 openings of m small polynomials over one domain in one call (keaki_hip_open_fk_poly_batch*, keaki_hip_vec_commit_batch*): the pipeline of
// fft_g1.hip's header with a row dimension. One call at d = 2^8 is ~67 launches whose butterflies fill 128 lanes; m rows pay every launch once.
//
// Point workspace, position-major: work[pos * M + row], M = the pass's row count rounded up to 64. A 64-lane workgroup is 64 rows of ONE
// position (butterfly): its 96-byte loads are contiguous across the wave and -- whatever the span -- it has ONE twiddle, so every stage runs the
// sliding-window ladder for a wave-uniform scalar (jac29.hip.h: jac_scalar_mul_uniform_u29_j) and no stage needs a per-lane table workspace.
// Lanes of the padding rows [rows, M) store nothing.
//   E[q] = (d a_row[2 brev(q)]) hat_s[q],  O[q] = a_row[2 brev(q) + 1] hat_s[d + q]      k_fkb_pointwise: the wave shares the POINT, the scalars are
//                                                                                        per lane: fixed-window ladder over ONE table in LDS
//   O <- DIT_d (inverse twiddles), O[i] <- w^-i O[i], O <- DIF_d                         k_fkb_stage<true>, k_fkb_twist, k_fkb_stage<false>
//   proofs[row][brev(q)] = affine(E[q] + O[q])                                           k_fkb_finish
// (a_row = DFT_2d(0..0, p_row) / 2d in natural order; hat_s: the handle's cached transform, positions as in fft_g1.hip.) The butterfly keeps the
// order of operations of k_g1_fft_stage_map: ladder, then j29_addsub with the generic additions for identities and u = +-v. An affine point is
// unique, so a row's proofs are the bytes keaki_hip_open_fk_poly returns for it. tests/fk_batch_model.py is this file over Z_q, index for index.
//
// Scalar side, rows as grid dimension y over row-major arrays (Fr arithmetic is exact): the size-d inverse transform with its 1/d (vec_commit
// only: evaluations [n, d) are zero) and the zero-prefixed size-2d transform with its 1/2d, one twiddle table per call.
#include <algorithm>
#include "ec_batch.hip.h"
#include "jac29.hip.h"
#include "internal.h"

namespace bn254 {

KDEV u32 fkb_brev(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
KDEV bool fkb_is_one(const Fr& a) {
  u32 o = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) o |= a.l[j] ^ FrParams::ONE[j];
  return o == 0;
}

// ---- scalar field, rows = gridDim.y -----------------------------------------------------------------------------------------------------------
// dst[row][brev(i)] = src[row * sstride + i - lo] for lo <= i < hi, zero elsewhere (i < 2^log2n): the input of an in-place transform
static __global__ void __launch_bounds__(256) k_fkb_fr_load(const Fr* __restrict__ src, size_t sstride, u32 lo, u32 hi, u32 log2n, Fr* __restrict__ dst) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x, n = 1u << log2n;
  if (i >= n) return;
  const size_t row = blockIdx.y;
  dst[row * n + fkb_brev(i, log2n)] = (i >= lo && i < hi) ? src[row * sstride + (i - lo)] : fp_zero<FrParams>();
}
// one radix-2 stage of span len; tw[k] = root^k for the root of order tw_n >= n
static __global__ void __launch_bounds__(256) k_fkb_fr_stage(Fr* __restrict__ a, const Fr* __restrict__ tw, u32 tw_n, u32 n, u32 len) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n / 2) return;
  a += (size_t)blockIdx.y * n;
  const u32 half = len >> 1, j = b % half, i0 = (b / half) * len + j, i1 = i0 + half;
  const Fr u = a[i0], v = fp_mul<FrParams>(a[i1], tw[(size_t)j * (tw_n / len)]);
  a[i0] = fp_add<FrParams>(u, v);
  a[i1] = fp_sub<FrParams>(u, v);
}
static __global__ void __launch_bounds__(256) k_fkb_fr_scale(Fr* __restrict__ a, Fr s, u32 total) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) a[i] = fp_mul<FrParams>(a[i], s);
}

// ---- group side: lane t of a launch is (position or butterfly t / M, row t % M) ------------------------------------------------------------------
// pos < d: E[pos], the scalar d a[2 brev(pos)]; pos >= d: O[pos - d], the scalar a[2 brev(pos - d) + 1]. a: rows x 2d, row-major.
// Every lane of the workgroup multiplies the SAME point: its window table {1..8} P is built once, in LDS (all lanes write the same words), and the
// fixed-window ladder of jac_scalar_mul_gtab_u29 reads it there by the lane's own digits.
static __global__ void __launch_bounds__(64) k_fkb_pointwise(const G1Jac* __restrict__ hs, const Fr* __restrict__ a, u32 log2d, u32 rows, u32 M,
                                                             G1Jac* __restrict__ work) {
  __shared__ uint4 tab[GTAB_UINT4_PER_LANE];
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x, d = 1u << log2d;
  const u32 pos = t / M, row = t % M;                      // pos < 2d (host: the grid is 2d M / 64 workgroups)
  const u32 part = pos >= d ? 1u : 0u, q = part ? pos - d : pos;
  const bool live = row < rows;                            // padding rows run the ladder on a zero scalar: the table build stays wave-wide
  Fr sc = fp_zero<FrParams>();
  if (live) sc = a[(size_t)row * 2 * d + 2 * (size_t)fkb_brev(q, log2d) + part];
  if (!part)
    for (u32 i = 0; i < log2d; i++) sc = fp_add<FrParams>(sc, sc);
  const G1Jac r = jac_scalar_mul_gtab_u29(hs[pos], sc, tab);
  if (live) work[(size_t)pos * M + row] = r;
}
// The radix-2 butterfly of k_g1_fft_stage_map<DIT, uniform, lazy add/sub> over the d positions of every row; tw[j * stride]: the twiddle of offset j
template <bool DIT>
static __global__ void __launch_bounds__(64, 3) k_fkb_stage(G1Jac* __restrict__ a, const Fr* __restrict__ tw, u32 half, u32 stride, u32 rows, u32 M) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 b = t / M, row = t % M;                        // b < d / 2 (host)
  if (row >= rows) return;
  const u32 j = b % half, blk = b / half;
  const size_t i0 = ((size_t)blk * 2 * half + j) * M + row, i1 = i0 + (size_t)half * M;
  const Fr w = tw[(size_t)j * stride];
  __shared__ unsigned char dig[2 * UNIFORM_DIG_STRIDE];
  auto addsub = [&](const G1Jac& u, bool v_inf, const J29& vj, G1Jac& sum, G1Jac& diff) {
    J29 sj, dj;
    if (!v_inf && !jac_is_inf(u) && j29_addsub(j29_from_sat(u), vj, sj, dj)) {
      sum = j29_to_sat(sj);
      diff = j29_to_sat(dj);
      return;
    }
    G1Jac v = v_inf ? jac_inf<Fq>() : j29_to_sat(vj);
    sum = jac_add(u, v);
    v.y = -v.y;
    diff = jac_add(u, v);
  };
  if (DIT) {
    const G1Jac v = a[i1];
    J29 vj;
    bool v_inf;
    if (fkb_is_one(w)) { v_inf = jac_is_inf(v); vj = j29_from_sat(v); }
    else v_inf = !jac_scalar_mul_uniform_u29_j(v, w, dig, vj);
    const G1Jac u = a[i0];
    G1Jac s_, d_;
    addsub(u, v_inf, vj, s_, d_);
    a[i0] = s_;
    a[i1] = d_;
  } else {
    const G1Jac u = a[i0], v = a[i1];
    G1Jac s_, t_;
    addsub(u, jac_is_inf(v), j29_from_sat(v), s_, t_);
    a[i0] = s_;
    if (!fkb_is_one(w)) {
      J29 tj;
      t_ = jac_scalar_mul_uniform_u29_j(t_, w, dig, tj) ? j29_to_sat(tj) : jac_inf<Fq>();
    }
    a[i1] = t_;
  }
}
// O[i] <- tw[i] O[i] (tw[i] = omega_2d^-i): one twiddle per workgroup
static __global__ void __launch_bounds__(64, 3) k_fkb_twist(G1Jac* __restrict__ o, const Fr* __restrict__ tw, u32 rows, u32 M) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 i = t / M, row = t % M;                        // i < d (host)
  if (row >= rows || i == 0) return;
  __shared__ unsigned char dig[2 * UNIFORM_DIG_STRIDE];
  const size_t at = (size_t)i * M + row;
  o[at] = jac_scalar_mul_uniform_u29(o[at], tw[i], dig);
}
// out[row * d + brev(q)] = affine(E[q] + O[q])
static __global__ void __launch_bounds__(64) k_fkb_finish(const G1Jac* __restrict__ e, const G1Jac* __restrict__ o, u32 log2d, u32 rows, u32 M,
                                                          G1Aff* __restrict__ out) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 q = t / M, row = t % M;                        // q < d (host)
  if (row >= rows) return;
  const size_t at = (size_t)q * M + row;
  out[((size_t)row << log2d) + fkb_brev(q, log2d)] = jac_to_aff(jac_add(e[at], o[at]));
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

static u32 fkb_pad64(size_t rows) { return (u32)((rows + 63) / 64 * 64); }
// rows of a pass: the workspaces of a pass stay below FKB_PASS_BYTES (whole workgroups of rows, at least one), at most FKB_ROWS_MAX (gridDim.y)
size_t fkb_rows_per_pass(u32 log2d, size_t m) {
  const size_t by_bytes = std::max<size_t>(64, FKB_PASS_BYTES / (FKB_ROW_BYTES << log2d) / 64 * 64);
  return std::min(m, std::min(by_bytes, FKB_ROWS_MAX));
}
// The two workspaces of a pass of `rows` rows: 2d M Jacobian points | hat_a (rows x 2d Fr), the coefficients of vec_commit (rows x d) and the
// three twiddle tables of the call (omega_2d^k, omega_2d^-k: k < d; omega_d^-k: k < d / 2)
static size_t fkb_pts_bytes(u32 log2d, size_t rows) { return ((size_t)2 << log2d) * fkb_pad64(rows) * sizeof(G1Jac); }
static size_t fkb_fr_bytes(u32 log2d, size_t rows) { return (rows * ((size_t)3 << log2d) + ((size_t)3 << log2d)) * sizeof(Fr); }
keaki_status fkb_reserve(keaki_hip_ctx* ctx, u32 log2d, size_t rows) {
  ST_TRY(reserve(ctx, ctx->fkb_pts, fkb_pts_bytes(log2d, rows)));
  return reserve(ctx, ctx->fkb_fr, fkb_fr_bytes(log2d, rows));
}
// the twiddle tables, at the end of the scalar workspace of a pass of `rows` rows (the layout of every pass of the call)
static Fr* fkb_tables_at(keaki_hip_ctx* ctx, u32 log2d, size_t rows) { return (Fr*)ctx->fkb_fr.p + rows * ((size_t)3 << log2d); }
const void* fkb_tables_run(keaki_hip_ctx* ctx, u32 log2d, size_t rows, const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* omega_d_inv) {
  const u32 d = 1u << log2d;
  Fr* tw = fkb_tables_at(ctx, log2d, rows);
  fr_powers_run(ctx, omega_2d, d, tw);
  fr_powers_run(ctx, omega_2d_inv, d, tw + d);
  if (omega_d_inv) fr_powers_run(ctx, omega_d_inv, std::max(1u, d / 2), tw + 2 * (size_t)d);
  return tw;
}
// in-place transforms of `rows` arrays of n = 2^log2n elements (already in bit-reversed order) and the scaling
static void fkb_fr_fft(keaki_hip_ctx* ctx, Fr* a, u32 log2n, u32 rows, const Fr* tw, u32 tw_n, const uint64_t* scale) {
  const u32 n = 1u << log2n;
  for (u32 len = 2; len <= n; len <<= 1)
    hipLaunchKernelGGL(k_fkb_fr_stage, dim3(cdiv(n / 2, 256), rows), dim3(256), 0, ctx->stream, a, tw, tw_n, n, len);
  Fr s;
  memcpy(&s, scale, 32);
  hipLaunchKernelGGL(k_fkb_fr_scale, dim3(cdiv((size_t)rows * n, 256)), dim3(256), 0, ctx->stream, a, s, rows * n);
}
// One pass: rows <= the count the workspaces were reserved for (`cap`). d_rows: row j at d_rows + j * stride (Fr): d coefficients, or with
// inv_d (vec_commit) the first n evaluations; then *d_coeffs_out = the rows' coefficients (rows x d, row-major) for the commitments.
// d_proofs: rows x d affine points. 1 <= log2d <= FKB_LOG2D_MAX.
keaki_status fkb_pass_run(keaki_hip_ctx* ctx, const void* d_hat_s, u32 log2d, size_t cap, const void* d_rows, size_t n, u32 rows, size_t stride,
                          const uint64_t* inv_d, const uint64_t* inv_2d, void* d_proofs, const void** d_coeffs_out) {
  const u32 d = 1u << log2d, M = fkb_pad64(rows);
  hipStream_t st = ctx->stream;
  Fr* hat_a = (Fr*)ctx->fkb_fr.p;
  Fr* coef = hat_a + (size_t)rows * 2 * d;
  const Fr *tw = fkb_tables_at(ctx, log2d, cap), *twi = tw + d, *twd = tw + 2 * (size_t)d;
  const Fr* p = (const Fr*)d_rows;
  size_t pstride = stride;
  if (inv_d) {
    hipLaunchKernelGGL(k_fkb_fr_load, dim3(cdiv(d, 256), rows), dim3(256), 0, st, (const Fr*)d_rows, stride, 0u, (u32)n, log2d, coef);
    fkb_fr_fft(ctx, coef, log2d, rows, twd, d, inv_d);
    p = coef;
    pstride = d;
    if (d_coeffs_out) *d_coeffs_out = coef;
  }
  hipLaunchKernelGGL(k_fkb_fr_load, dim3(cdiv(2 * d, 256), rows), dim3(256), 0, st, p, pstride, d, 2 * d, log2d + 1, hat_a);
  fkb_fr_fft(ctx, hat_a, log2d + 1, rows, tw, 2 * d, inv_2d);
  G1Jac *e = (G1Jac*)ctx->fkb_pts.p, *o = e + (size_t)d * M;
  const dim3 block(64), g_d(d * (M / 64)), g_half(d / 2 * (M / 64));
  hipLaunchKernelGGL(k_fkb_pointwise, dim3(2 * d * (M / 64)), block, 0, st, (const G1Jac*)d_hat_s, (const Fr*)hat_a, log2d, rows, M, e);
  for (u32 half = 1; half <= d / 2; half <<= 1)
    hipLaunchKernelGGL(k_fkb_stage<true>, g_half, block, 0, st, o, twi, half, 2 * (d / (2 * half)), rows, M);
  hipLaunchKernelGGL(k_fkb_twist, g_d, block, 0, st, o, twi, rows, M);
  for (u32 half = d / 2; half >= 1; half >>= 1)
    hipLaunchKernelGGL(k_fkb_stage<false>, g_half, block, 0, st, o, tw, half, 2 * (d / (2 * half)), rows, M);
  hipLaunchKernelGGL(k_fkb_finish, g_d, block, 0, st, (const G1Jac*)e, (const G1Jac*)o, log2d, rows, M, (G1Aff*)d_proofs);
  return launch_check(ctx, "fk_batch");
}

}  // namespace keaki_internal
