// KZG set batch verification (keaki_hip_kzg_verify_sets): the scalar-field side. Item i < n is a set of k DISTINCT points z_(i,0) .. z_(i,k-1) with k
// claimed values y_(i,j) = p_i(z_(i,j)), a proof and the caller's gamma_i. With Z_i(X) = prod_j (X - z_(i,j)) = sum_(t <= k) Z_(i,t) X^t (monic) and
// I_i(X) = sum_(t < k) I_(i,t) X^t the interpolant of (z_(i,j), y_(i,j)), what the group side of the call (api.hip) needs from here:
//     S        k + 1 rows of n scalars, row t at S + 32 (t n + i) bytes (the layout the batched MSM takes, stride n): row 0 = -gamma_i Z_(i,0),
//              rows 1 .. k - 1 = gamma_i Z_(i,t), row k = gamma_i (Z_(i,k) = 1)
//     -J_t     = -sum_i gamma_i I_(i,t)  (t < k: the scalars of the MSM over [tau^t]_1)          g = sum gamma_i  (com_stride 0: the scalar of C)
//   k_vs_points   point_mode 1 only: z = omega^idx for every (item, j), one lane per pair, so that every later kernel reads Fr. (A launch of its own, not
//                 the head of k_vs_weights: a lane of that kernel needs ALL k points of its items, which other lanes -- of other workgroups -- derive.)
//   k_vs_weights  w_(i,j) = 1 / Z_i'(z_(i,j)) = 1 / prod_(t != j) (z_(i,j) - z_(i,t)). A lane owns VS_INV = 16 consecutive (item, j) pairs, forms their k - 1
//                 products each and inverts all 16 with ONE Fermat inversion (prefix products up, one inversion, back down, as k_vc_prepare): 3 products
//                 + 1/16 of ~380 per pair on top of the k - 1. The products wait in the rows of S, which k_vs_polys writes only afterwards. A repeated
//                 point zeroes a product and with it the prefix products behind it: the weights of the 16 pairs of that lane come out 0 (distinct points
//                 are the caller's contract, as for set_polys).
//   k_vs_polys    ONE launch, grid-stride over tiles. kp = the power of two >= k; a workgroup of 256 lanes takes T = 256 / kp items a tile, lane
//                 (slot, c) = (tid / kp, tid % kp). Z by k steps through LDS (new[c] = old[c - 1] - z_j old[c]), I by the skewed synthetic division of
//                 k_set_polys (lane j divides Z by (X - z_j) from the top, started j steps late, so that in every step the lanes of a slot add into
//                 DIFFERENT coefficients: 2k - 1 steps, no reduction), both for all T slots side by side. Then lane (slot, c) writes its entry of row c
//                 (lane c = 0 also row k) and adds gamma_i I_(i,c) to a register it keeps over all tiles of the workgroup. After the last tile the T slots
//                 are folded (a tree in LDS) and the workgroup writes ONE row of k partial sums and its partial of g. Every barrier is uniform: lanes
//                 past n or past k are masked, never skipped.
//   k_vs_finish   folds the rows of all workgroups (one workgroup of 1,024 lanes: a wave takes every sixteenth row, a lane a column) into -J and g.
// Fr sums are exact: neither the tiling nor the number of workgroups changes a bit of the result.
// LDS: three arrays of 256 Fr (points, Z, I), each in TWO planes of 16 B (words 0 - 3, words 4 - 7) as in kzg_cosets.hip: neighbouring lanes read
// neighbouring 16-byte slots (the neighbour's coefficient, the own slot), the lanes of one slot read ONE address (z_j: a broadcast), and in a step of I the
// lanes of a slot hit consecutive coefficients. 24 KB a workgroup.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this file; no kernel uses scratch memory or atomics):
//   k_vs_points   48 VGPRs, no LDS           k_vs_weights  80 VGPRs, no LDS
//   k_vs_polys<0>  140 VGPRs, 24,576 B LDS    k_vs_finish   70 VGPRs, 33,280 B LDS    k_vs_pairs  33 VGPRs, no LDS
//   k_vs_polys<1>, <2> (the rows of kzg set_pairs: no gammas, no partial sums)  112 VGPRs, 24,576 B LDS
#include <algorithm>
#include "internal.h"
#include "bn254_curve.hip.h"
#include "kzg_fr.hip.h"

namespace bn254 {

constexpr u32 VS_THREADS = 256;
constexpr u32 VS_INV = 16;                                  // (item, j) pairs per Fermat inversion
constexpr u32 VS_FIN_THREADS = 1024, VS_FIN_WAVES = VS_FIN_THREADS / 64;
constexpr u32 VS_COLS_MAX = KEAKI_VERIFY_SETS_K_MAX + 1;    // columns of a partial row: k sums of J and one of g

// 256 Fr in two 16-byte planes
struct VsArr {
  uint4 lo[VS_THREADS], hi[VS_THREADS];
};
KDEV Fr vs_ld(const VsArr& a, u32 p) {
  const uint4 x = a.lo[p], y = a.hi[p];
  Fr r;
  r.l[0] = x.x; r.l[1] = x.y; r.l[2] = x.z; r.l[3] = x.w;
  r.l[4] = y.x; r.l[5] = y.y; r.l[6] = y.z; r.l[7] = y.w;
  return r;
}
KDEV void vs_st(VsArr& a, u32 p, const Fr& v) {
  a.lo[p] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  a.hi[p] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// pts[i k + j] = omega^idx[i item_stride + j]
static __global__ void __launch_bounds__(VS_THREADS) k_vs_points(const u32* __restrict__ idx, u64 item_stride, Fr omega, u32 n, u32 k, Fr* __restrict__ pts) {
  const u32 total = n * k, lanes = gridDim.x * VS_THREADS;
#pragma unroll 1
  for (u32 e = blockIdx.x * VS_THREADS + threadIdx.x; e < total; e += lanes) {
    const u32 i = e / k, j = e - i * k;
    pts[e] = fr_pow_u32(omega, idx[(u64)i * item_stride + j]);
  }
}

// w[i k + j] = 1 / prod_(t != j) (z_(i,j) - z_(i,t)), z_(i,j) at z + i zstride + j. Grid-stride over the chunks of VS_INV pairs; w and `keep` (n k
// Fr: the products on the way up) double as the lane's own scratch.
static __global__ void __launch_bounds__(VS_THREADS) k_vs_weights(const Fr* __restrict__ z, u64 zstride, u32 n, u32 k, Fr* __restrict__ w, Fr* __restrict__ keep) {
  const u32 total = n * k, chunks = (total + VS_INV - 1) / VS_INV, lanes = gridDim.x * VS_THREADS;
#pragma unroll 1
  for (u32 c = blockIdx.x * VS_THREADS + threadIdx.x; c < chunks; c += lanes) {
    const u32 e0 = c * VS_INV, m = min(VS_INV, total - e0);
    Fr pre = fp_one<FrParams>();
#pragma unroll 1
    for (u32 s = 0; s < m; s++) {                   // up: w[e] = d_e0 .. d_e
      const u32 e = e0 + s, i = e / k, j = e - i * k;
      const Fr* zi = z + (u64)i * zstride;
      const Fr zj = zi[j];
      Fr d = fp_one<FrParams>();
#pragma unroll 1
      for (u32 t = 0; t < k; t++)
        if (t != j) d = fp_mul<FrParams>(d, fp_sub<FrParams>(zj, zi[t]));
      keep[e] = d;
      pre = fp_mul<FrParams>(pre, d);
      w[e] = pre;
    }
    Fr inv = fr_inv(pre);                           // 1 / (d_e0 .. d_(e0 + m - 1))
#pragma unroll 1
    for (u32 s = m; s-- > 0;) {                     // down
      const u32 e = e0 + s;
      const Fr d = keep[e];
      w[e] = s ? fp_mul<FrParams>(inv, w[e - 1]) : inv;
      inv = fp_mul<FrParams>(inv, d);
    }
  }
}

// rows: S[t n + i] as in the file header; part[blockIdx.x (k + 1) + t] = sum over the items i of this workgroup's tiles of gamma_i I_(i,t) (t < k),
// and of gamma_i (t = k). z_(i,j) at z + i zstride + j, y_(i,j) at y + i ystride + j, w dense (i k + j).
// ROWS != 0 (kzg set_pairs: no gammas, no partial sums, no k_vs_finish): S[(i << log2kp) + t] = -I_(i,t) for t < k and zero up to kp (the layout k_cp_rows
// reads; canonical integers, ROWS = 2: the Montgomery form the batched MSM takes) and part[i k + t] = Z_(i,t), t < k, canonical (the monic top coefficient is
// not stored).
template <int ROWS>
static __global__ void __launch_bounds__(VS_THREADS) k_vs_polys(const Fr* __restrict__ z, u64 zstride, const Fr* __restrict__ y, u64 ystride, const Fr* __restrict__ w,
                                                                const Fr* __restrict__ gammas, u32 n, u32 k, u32 log2kp, Fr* __restrict__ S, Fr* __restrict__ part) {
  __shared__ VsArr pz, zc, ic;
  const u32 tid = threadIdx.x;
  const u32 kp = 1u << log2kp, log2T = 8u - log2kp, T = 1u << log2T;
  const u32 slot = tid >> log2kp, c = tid & (kp - 1), base = slot << log2kp;
  const u32 tiles = (n + T - 1) >> log2T;
  Fr acc = fp_zero<FrParams>(), accg = fp_zero<FrParams>();

#pragma unroll 1
  for (u32 q = blockIdx.x; q < tiles; q += gridDim.x) {
    const u32 item = (q << log2T) + slot;
    const bool live = item < n && c < k;
    const Fr zme = live ? z[(u64)item * zstride + c] : fp_zero<FrParams>();
    vs_st(pz, tid, zme);
    __syncthreads();
    // Z: the running product, monic of degree j before step j (lane j holds the leading 1 while j < k)
    Fr cur = c == 0 ? fp_one<FrParams>() : fp_zero<FrParams>();
#pragma unroll 1
    for (u32 j = 0; j < k; j++) {
      const Fr zj = vs_ld(pz, base + j);
      vs_st(zc, tid, cur);
      __syncthreads();
      const Fr prev = c ? vs_ld(zc, tid - 1) : fp_zero<FrParams>();
      cur = fp_sub<FrParams>(prev, fp_mul<FrParams>(zj, cur));
      __syncthreads();
    }
    vs_st(zc, tid, cur);
    vs_st(ic, tid, fp_zero<FrParams>());
    // I: lane c is at coefficient idx = k - 1 - (step - c) of its quotient Z / (X - z_c) in step `step`
    const Fr s = live ? fp_mul<FrParams>(y[(u64)item * ystride + c], w[(size_t)item * k + c]) : fp_zero<FrParams>();
    Fr qc = fp_one<FrParams>();
    __syncthreads();
#pragma unroll 1
    for (u32 step = 0; step + 1 < 2 * k; step++) {
      if (live && step >= c && step - c < k) {
        const u32 idx = k - 1 - (step - c);
        if (step > c) qc = fp_add<FrParams>(vs_ld(zc, base + idx + 1), fp_mul<FrParams>(zme, qc));
        vs_st(ic, base + idx, fp_add<FrParams>(vs_ld(ic, base + idx), fp_mul<FrParams>(s, qc)));
      }
      __syncthreads();
    }
    if constexpr (ROWS != 0) {
      if (item < n) {
        Fr ni = fp_zero<FrParams>(), out;
        if (c < k) ni = fp_neg<FrParams>(vs_ld(ic, tid));
        if (ROWS == 2) out = ni;
        else fp_from_mont<FrParams>(out.l, ni);
        S[((size_t)item << log2kp) + c] = out;
        if (c < k) {
          fp_from_mont<FrParams>(out.l, cur);
          part[(size_t)item * k + c] = out;
        }
      }
      __syncthreads();
      continue;
    }
    if (live) {
      const Fr gamma = gammas[item];
      Fr row = fp_mul<FrParams>(gamma, cur);
      if (c == 0) {
        row = fp_neg<FrParams>(row);
        S[(size_t)k * n + item] = gamma;
        accg = fp_add<FrParams>(accg, gamma);
      }
      S[(size_t)c * n + item] = row;
      acc = fp_add<FrParams>(acc, fp_mul<FrParams>(gamma, vs_ld(ic, tid)));
    }
    __syncthreads();                                // the next tile overwrites the three arrays
  }

  if constexpr (ROWS != 0) return;
  // fold the T slots: entry slot * kp + c, a tree over the slots; then the same tree down to one entry for g
  vs_st(ic, tid, acc);
  vs_st(zc, tid, accg);
  __syncthreads();
#pragma unroll 1
  for (u32 h = VS_THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      if (h >= kp) vs_st(ic, tid, fp_add<FrParams>(vs_ld(ic, tid), vs_ld(ic, tid + h)));
      vs_st(zc, tid, fp_add<FrParams>(vs_ld(zc, tid), vs_ld(zc, tid + h)));
    }
    __syncthreads();
  }
  Fr* row = part + (size_t)blockIdx.x * (k + 1);
  if (tid < k) row[tid] = vs_ld(ic, tid);
  if (tid == 0) row[k] = vs_ld(zc, 0);
}

// neg_j[t] = -sum over the `blocks` rows of part (t < k), g_out = the sum of their last column. ONE workgroup: wave v takes the rows v, v + 16, ..,
// a lane the columns lane and lane + 64 (k + 1 <= 65 of them); LDS folds the sixteen.
static __global__ void __launch_bounds__(VS_FIN_THREADS) k_vs_finish(const Fr* __restrict__ part, u32 blocks, u32 k, Fr* __restrict__ neg_j, Fr* __restrict__ g_out) {
  __shared__ Fr sh[VS_FIN_WAVES * VS_COLS_MAX];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, cols = k + 1;
#pragma unroll 1
  for (u32 col = lane; col < cols; col += 64u) {
    Fr sum = fp_zero<FrParams>();
#pragma unroll 4
    for (u32 b = wave; b < blocks; b += VS_FIN_WAVES) sum = fp_add<FrParams>(sum, part[(size_t)b * cols + col]);
    sh[wave * VS_COLS_MAX + col] = sum;
  }
  __syncthreads();
  const u32 col = threadIdx.x;
  if (col < cols) {
    Fr sum = sh[col];
#pragma unroll 1
    for (u32 v = 1; v < VS_FIN_WAVES; v++) sum = fp_add<FrParams>(sum, sh[v * VS_COLS_MAX + col]);
    if (col < k) neg_j[col] = fp_neg<FrParams>(sum);
    else *g_out = sum;
  }
}

// The k + 1 sums of the call as the pairings take them: sums_aff[0] = L, sums_aff[t] = R_t = rows_jac[t] (1 <= t <= k), affine with (0, 0) for the
// identity (all inputs are normalised Jacobian points: no arithmetic but one negation), and ps = the same with -L in front.
static __global__ void __launch_bounds__(128) k_vs_pairs(const Fq* __restrict__ l_jac, const Fq* __restrict__ rows_jac, u32 k, G1Aff* __restrict__ sums_aff,
                                                         G1Aff* __restrict__ ps) {
  const u32 t = threadIdx.x;
  if (blockIdx.x != 0 || t > k) return;
  const Fq* p = t ? rows_jac + 3 * (size_t)t : l_jac;
  const bool inf = f_is_zero(p[2]);
  G1Aff a;
  a.x = inf ? fq_zero() : p[0];
  a.y = inf ? fq_zero() : p[1];
  sums_aff[t] = a;
  if (t == 0 && !inf) a.y = -a.y;
  ps[t] = a;
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

namespace {
u32 vs_log2kp(size_t k) { u32 b = 0; while (((size_t)1 << b) < k) b++; return b; }
u32 vs_tiles(size_t n, size_t k) { return cdiv(n, VS_THREADS >> vs_log2kp(k)); }
u32 vs_rows_max(size_t n, size_t k) { return std::min<u32>(vs_tiles(n, k), VS_MAX_BLOCKS); }
}  // namespace

// [S: (k + 1) n | w: n k | -J: K_MAX | g: 1 | part: rows x (k + 1) | pts: n k, point_mode 1 only] Fr
size_t verify_sets_work_bytes(size_t n, size_t k, int point_mode) {
  return ((k + 1) * n + n * k + KEAKI_VERIFY_SETS_K_MAX + 1 + (size_t)vs_rows_max(n, k) * (k + 1) + (point_mode ? n * k : 0)) * sizeof(Fr);
}
VsWork verify_sets_layout(size_t n, size_t k, void* d_work) {
  Fr* p = (Fr*)d_work;
  VsWork w;
  w.s = p; p += (k + 1) * n;
  w.w = p; p += n * k;
  w.neg_j = p; p += KEAKI_VERIFY_SETS_K_MAX;
  w.g = p; p += 1;
  w.part = p; p += (size_t)vs_rows_max(n, k) * (k + 1);
  w.pts = p;
  return w;
}

keaki_status verify_sets_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const uint64_t* omega, const void* d_values,
                                     size_t item_stride, size_t k, size_t n, const VsWork& w) {
  if (n == 0 || k == 0 || k > KEAKI_VERIFY_SETS_K_MAX || item_stride < k || n * k >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_verify_sets: n = %zu items of %zu points out of range on the device side", n, k);
  const u32 total = (u32)(n * k);
  const Fr* z = (const Fr*)d_points;
  u64 zstride = item_stride;
  if (point_mode) {
    Fr om;
    memcpy(&om, omega, 32);
    hipLaunchKernelGGL(k_vs_points, dim3(std::min<u32>(cdiv(total, VS_THREADS), ctx->n_cu * 8u)), dim3(VS_THREADS), 0, ctx->stream, (const u32*)d_points,
                       (u64)item_stride, om, (u32)n, (u32)k, (Fr*)w.pts);
    z = (const Fr*)w.pts;
    zstride = k;
  }
  hipLaunchKernelGGL(k_vs_weights, dim3(std::min<u32>(cdiv(cdiv(total, VS_INV), VS_THREADS), ctx->n_cu * 8u)), dim3(VS_THREADS), 0, ctx->stream, z, zstride, (u32)n,
                     (u32)k, (Fr*)w.w, (Fr*)w.s);
  // 140 VGPRs a lane: three workgroups (one wave per SIMD each) per compute unit; the rows the workspace holds bound the grid
  const int opt = ctx->tune.verify_sets_blocks;
  const u32 cap = opt > 0 ? (u32)opt : ctx->n_cu * 3u;
  const u32 blocks = std::min<u32>(vs_rows_max(n, k), cap);
  hipLaunchKernelGGL(k_vs_polys<0>, dim3(blocks), dim3(VS_THREADS), 0, ctx->stream, z, zstride, (const Fr*)d_values, (u64)item_stride, (const Fr*)w.w,
                     (const Fr*)d_gammas, (u32)n, (u32)k, vs_log2kp(k), (Fr*)w.s, (Fr*)w.part);
  hipLaunchKernelGGL(k_vs_finish, dim3(1), dim3(VS_FIN_THREADS), 0, ctx->stream, (const Fr*)w.part, blocks, (u32)k, (Fr*)w.neg_j, (Fr*)w.g);
  return launch_check(ctx, "verify_sets_scalars");
}

// kzg set_pairs: the rows of the m items [first, first + m) of the caller's arrays (internal.h). The same three kernels on the chunk's part of the arrays; the
// products of k_vs_weights wait in d_rows_i (m kp >= m k Fr), which the rows kernel writes only afterwards.
keaki_status set_pairs_rows_run(keaki_hip_ctx* ctx, const void* d_points, int point_mode, const uint64_t* omega, const void* d_values, size_t item_stride, size_t k,
                                size_t first, size_t m, bool mont, void* d_w, void* d_pts, void* d_rows_i, void* d_rows_z) {
  const u32 log2kp = vs_log2kp(k);
  if (m == 0 || k == 0 || k > KEAKI_VERIFY_SETS_K_MAX || item_stride < k || (m << log2kp) >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_set_pairs: a chunk of %zu items of %zu points out of range on the device side", m, k);
  const u32 total = (u32)(m * k);
  const Fr* z = (const Fr*)d_points + first * item_stride;
  u64 zstride = item_stride;
  if (point_mode) {
    Fr om;
    memcpy(&om, omega, 32);
    hipLaunchKernelGGL(k_vs_points, dim3(std::min<u32>(cdiv(total, VS_THREADS), ctx->n_cu * 8u)), dim3(VS_THREADS), 0, ctx->stream,
                       (const u32*)d_points + first * item_stride, (u64)item_stride, om, (u32)m, (u32)k, (Fr*)d_pts);
    z = (const Fr*)d_pts;
    zstride = k;
  }
  hipLaunchKernelGGL(k_vs_weights, dim3(std::min<u32>(cdiv(cdiv(total, VS_INV), VS_THREADS), ctx->n_cu * 8u)), dim3(VS_THREADS), 0, ctx->stream, z, zstride, (u32)m,
                     (u32)k, (Fr*)d_w, (Fr*)d_rows_i);
  const u32 blocks = std::min<u32>(vs_tiles(m, k), ctx->n_cu * 3u);
  const Fr* y = (const Fr*)d_values + first * item_stride;
  if (mont)
    hipLaunchKernelGGL(k_vs_polys<2>, dim3(blocks), dim3(VS_THREADS), 0, ctx->stream, z, zstride, y, (u64)item_stride, (const Fr*)d_w, (const Fr*)nullptr, (u32)m,
                       (u32)k, log2kp, (Fr*)d_rows_i, (Fr*)d_rows_z);
  else
    hipLaunchKernelGGL(k_vs_polys<1>, dim3(blocks), dim3(VS_THREADS), 0, ctx->stream, z, zstride, y, (u64)item_stride, (const Fr*)d_w, (const Fr*)nullptr, (u32)m,
                       (u32)k, log2kp, (Fr*)d_rows_i, (Fr*)d_rows_z);
  return launch_check(ctx, "set_pairs_rows");
}

keaki_status verify_sets_pairs_run(keaki_hip_ctx* ctx, const void* d_l_jac, const void* d_rows_jac, size_t k, void* d_sums_aff, void* d_ps_aff) {
  if (k == 0 || k > KEAKI_VERIFY_SETS_K_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "verify_sets_pairs: k = %zu out of range", k);
  hipLaunchKernelGGL(k_vs_pairs, dim3(1), dim3(128), 0, ctx->stream, (const Fq*)d_l_jac, (const Fq*)d_rows_jac, (u32)k, (G1Aff*)d_sums_aff, (G1Aff*)d_ps_aff);
  return launch_check(ctx, "verify_sets_pairs");
}

}  // namespace keaki_internal
