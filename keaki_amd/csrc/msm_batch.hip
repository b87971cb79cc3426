// Batched small MSM over one SRS, and the batched quotient of `open`: m polynomials of n <= N_BATCH_MAX coefficients in one call
// (keaki_hip_msm_g1_batch*, keaki_hip_kzg_open_batch*; generalises commit / open, reference src/kzg.rs:89-101 and :104-124, to m rows).
//
//     out[j] = sum_{i<n} scalars[j][i] * srs[i],  j < m        each the normalised Jacobian point keaki_hip_msm_g1 returns
//
// The single-MSM pipeline (msm_host.hip.h) is ~15 launches whose floor is latency (0.4 .. 2.3 ms a call whatever n is); m calls pay it m times.
// Here the whole batch is three launches:
//   k_mb_canon     one lane per scalar: Montgomery -> canonical integer, plus the plan's BIAS (below). 32 B in, 32 B out.
//   k_mb_windows   grid (window groups, rows). A workgroup of 256 lanes owns G = 256 / B consecutive windows of ONE row, B = 2^(c-1) buckets each:
//                  lane t is slot (window t / B, bucket t % B). The n * G digits are counting-sorted by slot in LDS (count, scan, place: 2-byte
//                  entries index | sign << 15), every lane adds up its bucket with the XYZZ mixed addition in the lazy 29-bit limbs (the loop of
//                  k_msm_accumulate_g1_u29 without its chunk states: equal operands double, opposite operands empty the bucket), and the B
//                  buckets of a window are reduced to sum_b (b + 1) S_b by a weighted binary tree inside the workgroup: a node over the buckets
//                  [lo, lo + 2^k) carries A = sum S_b and Wt = sum (b - lo) S_b; two children merge as A = A_l + A_r,
//                  Wt = Wt_l + Wt_r + 2^k A_r. The window sum A + Wt of every (row, window) goes to a workspace (128 B).
//   k_mb_close     one lane per row: Horner over the W window sums from the top (acc = 2^width(w) acc + S_w) and ONE normalisation, so the serial
//                  chain of ~254 doublings is paid once per batch, not once per polynomial.
//
// Plan and digits. The window plan is msm_make_plan(n, c) with c chosen from n alone (msm_batch_window: the smallest c in 4 .. 9 with
// n / 2^(c-1) <= 16, i.e. about sixteen points per bucket; 9 above 2,048). Every window of those plans has at most B = 2^(c-1) buckets (signed
// digits below the top window, which is c - 1 bits wide and unsigned), so a window always fits its B slots. Signed digits without a carry chain:
// k_mb_canon stores v' = v + BIAS, BIAS = sum_{w < W-1} 2^(width(w) - 1) 2^(offset(w)). Then with u_w = (v' >> offset(w)) mod 2^width(w)
//     v = sum_{w < W-1} (u_w - 2^(width(w)-1)) 2^offset(w) + u_(W-1) 2^offset(W-1)
// so the digit of a signed window is u_w - half in [-half, half - 1] (bucket |d| - 1, zero digits skipped) and the carries of the classical
// recoding -- into the top window included -- are the carries of that one 256-bit addition. v < r and BIAS < 2^offset(W-1) keep the top digit at
// or below r / 2^offset(W-1) + 1 < 2^(c-1) = B.
//
// Limit: N_BATCH_MAX = 16,384 coefficients -- the 2-byte entries of the LDS sort hold a 14-bit index, and 16,384 entries are its 32 KB. Longer
// rows, and batches whose workspace the allocation limit refuses, run the single-MSM pipeline row by row (msm_g1_run, unchanged): every n is
// covered and the result does not depend on the route. The batch path reads the SRS points only, never the window tables of the handle; a handle
// with tables and one without give the same bytes because the normalised result is unique.
//
// k_fr_quotient_batch: q_j = (p_j - p_j(z_j)) / (x - z_j) and p_j(z_j) for m rows in one launch, one workgroup per row, by the recurrence of
// keaki_hip_kzg_quotient (Q_i = c_i + z Q_(i+1); fft_g1.hip) cut into 256 segments: local Horner values, one lane chains the 256 carries, every
// lane re-runs its segment from its carry. Fr arithmetic is exact and canonical, so the values equal those of the single call bit for bit.
#include <algorithm>
#include "internal.h"
#include "msm.hip.h"

namespace bn254 {

constexpr u32 MB_THREADS = 256;                 // lanes of a k_mb_windows workgroup = its (window, bucket) slots
constexpr u32 MB_N_MAX = 16384;                 // N_BATCH_MAX: 14-bit index in a 2-byte entry
constexpr u32 MB_C_MIN = 4, MB_C_MAX = 9;       // B = 8 .. 256 buckets per window
constexpr u32 MB_PAIRS_MAX = 16384;             // digits a workgroup sorts (n * G): 32 KB of LDS
constexpr u32 MB_SIGN = 0x8000u, MB_NONE = 0xFFFFFFFFu;
struct MbBias { u32 l[8]; };

static __global__ void __launch_bounds__(256) k_mb_canon(const Fr* __restrict__ scalars, u32 n, u32 rows, size_t stride, MbBias bias,
                                                         u32* __restrict__ canon) {
  const u32 total = rows * n;                   // < 2^31 (api.hip)
  for (u32 g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
    const u32 row = g / n, i = g - row * n;
    u32 v[8];
    fp_from_mont<FrParams>(v, scalars[(size_t)row * stride + i]);
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      carry += (u64)v[j] + bias.l[j];
      v[j] = (u32)carry;
      carry >>= 32;
    }
    uint4* dst = (uint4*)(canon + (size_t)g * 8);
    dst[0] = make_uint4(v[0], v[1], v[2], v[3]);
    dst[1] = make_uint4(v[4], v[5], v[6], v[7]);
  }
}

// digit of window w of the biased scalar at sc[0..8): bucket | sign << 15, MB_NONE for a zero digit
KDEV u32 mb_digit(const u32* __restrict__ sc, const MsmShape& s, u32 w) {
  const u32 off = msm_bit_offset(s, w), wd = msm_width(s, w), j = off >> 5, sh = off & 31u;
  const u32 lo = sc[j], hi = j + 1 < 8 ? sc[j + 1] : 0u;
  const u32 u = (u32)((((u64)hi << 32) | lo) >> sh) & ((1u << wd) - 1u);
  if (w == s.W - 1) return u ? u - 1u : MB_NONE;
  const u32 half = 1u << (wd - 1);
  if (u == half) return MB_NONE;
  return u > half ? u - half - 1u : ((half - u - 1u) | MB_SIGN);
}

static __global__ void __launch_bounds__(MB_THREADS, 2) k_mb_windows(const G1Aff* __restrict__ points, const u32* __restrict__ canon, MsmShape s, u32 logB,
                                                                    Xyzz<Fq>* __restrict__ wsums) {
  __shared__ u32 cnt[MB_THREADS], start[MB_THREADS];
  // the sorted entries during the bucket loop, the tree's mailboxes after it (level 0: 128 x A; level k: 2^(7-k) x (A, Wt))
  __shared__ __attribute__((aligned(16))) unsigned char pool[MB_PAIRS_MAX * 2];
  static_assert(sizeof(X29) * (MB_THREADS / 2) <= MB_PAIRS_MAX * 2, "the tree's mailboxes fit the sort's pool");
  u16* idx = (u16*)pool;
  X29* box = (X29*)pool;
  const u32 t = threadIdx.x, row = blockIdx.y, B = 1u << logB, G = MB_THREADS >> logB, w0 = blockIdx.x * G;
  const u32 wn = min(G, s.W - w0);                               // windows of this group that exist
  const u32* __restrict__ sc = canon + (size_t)row * s.n * 8;
  cnt[t] = 0;
  __syncthreads();
  for (u32 i = t; i < s.n; i += MB_THREADS)
    for (u32 g = 0; g < wn; g++) {
      const u32 code = mb_digit(sc + (size_t)i * 8, s, w0 + g);
      if (code != MB_NONE) atomicAdd(&cnt[(g << logB) + (code & (MB_SIGN - 1u))], 1u);
    }
  __syncthreads();
  const u32 mine = cnt[t];
  start[t] = mine;
  __syncthreads();
  for (u32 o = 1; o < MB_THREADS; o <<= 1) {                     // inclusive scan of the 256 counts
    const u32 v = t >= o ? start[t - o] : 0u;
    __syncthreads();
    start[t] += v;
    __syncthreads();
  }
  const u32 base = start[t] - mine;
  __syncthreads();
  start[t] = base;
  cnt[t] = 0;
  __syncthreads();
  for (u32 i = t; i < s.n; i += MB_THREADS)
    for (u32 g = 0; g < wn; g++) {
      const u32 code = mb_digit(sc + (size_t)i * 8, s, w0 + g);
      if (code == MB_NONE) continue;
      const u32 key = (g << logB) + (code & (MB_SIGN - 1u));
      idx[start[key] + atomicAdd(&cnt[key], 1u)] = (u16)(i | (code & MB_SIGN));
    }
  __syncthreads();
  // ---- bucket t: `mine` entries from idx[base]; the mixed addition of k_msm_accumulate_g1_u29, the next row requested an iteration ahead ----
  U29 X1, Y1, ZZ, ZZZ;
  bool empty = true;
  u32 e1 = mine ? idx[base] : 0u;
  G1Aff q1 = points[e1 & (MB_SIGN - 1u)];
#pragma unroll 1
  for (u32 k = 0; k < mine; k++) {
    const u32 e = e1;
    G1Aff q = q1;
    if (k + 1 < mine) {
      e1 = idx[base + k + 1];
      q1 = points[e1 & (MB_SIGN - 1u)];
    }
    if (aff_is_inf(q)) continue;
    q.y = f_cneg(q.y, (e & MB_SIGN) != 0);
    const U29 X2 = u29_from_sat_shift5(q.x.l), Y2 = u29_from_sat_shift5(q.y.l);
    if (empty) {
      X1 = u29_mul(X2, u29_one());
      Y1 = u29_mul(Y2, u29_one());
      ZZ = u29_one();
      ZZZ = u29_one();
      empty = false;
      continue;
    }
    const U29 U2 = u29_mul(X2, ZZ), S2 = u29_mul(Y2, ZZZ);
    const U29 P = u29_sub(U2, X1, Q29::K16), R = u29_sub(S2, Y1, Q29::K4);
    if (u29_maybe_zero(P)) {
      if (u29_is_zero(P)) {
        if (u29_is_zero(R)) {           // the same point again: double it in the saturated arithmetic, re-enter
          Xyzz<Fq> d = xyzz_dbl_aff(q);
          X1 = u29_from_fq(d.x); Y1 = u29_from_fq(d.y); ZZ = u29_from_fq(d.zz); ZZZ = u29_from_fq(d.zzz);
        } else {
          empty = true;                 // opposite points: the bucket is the identity again
        }
        continue;
      }
    }
    const U29 PP = u29_sqr(P), PPP = u29_mul(P, PP), Q = u29_mul(X1, PP);
    const U29 X3 = u29_sub3(u29_sqr(R), PPP, Q);
    const U29 T = u29_sub(Q, X3, Q29::K16);
    U29 NY1;
#pragma unroll
    for (int i = 0; i < 9; i++) NY1.l[i] = Q29::K2[i] - Y1.l[i];
    Y1 = u29_mul2(R, T, NY1, PPP);
    X1 = X3;
    ZZ = u29_mul(ZZ, PP);
    ZZZ = u29_mul(ZZZ, PPP);
  }
  // the bucket leaves the loop canonical and re-enters the tail form, as between k_msm_accumulate_g1_u29 and the MSM tail
  X29 A = x29_inf();
  if (!empty) {
    Xyzz<Fq> b;
    b.x = u29_to_fq(X1); b.y = u29_to_fq(Y1); b.zz = u29_to_fq(ZZ); b.zzz = u29_to_fq(ZZZ);
    A = x29_load(b);
  }
  X29 Wt = x29_inf();
  __syncthreads();                      // every lane is done with idx: the pool becomes the tree's mailboxes
#pragma unroll 1
  for (u32 k = 0; k < logB; k++) {
    const u32 o = 1u << k, pos = t & (2u * o - 1u), slot = (t >> (k + 1)) * (k ? 2u : 1u);
    if (pos == o) {
      box[slot] = A;
      if (k) box[slot + 1] = Wt;
    }
    __syncthreads();
    if (pos == 0) {
      const X29 Ar = box[slot];
      X29 sh = Ar;
#pragma unroll 1
      for (u32 d = 0; d < k; d++) sh = x29_dbl(sh);
      if (k) Wt = x29_add(x29_add(Wt, box[slot + 1]), sh);
      else Wt = sh;
      A = x29_add(A, Ar);
    }
    __syncthreads();
  }
  if ((t & (B - 1u)) == 0 && (t >> logB) < wn) wsums[(size_t)row * s.W + w0 + (t >> logB)] = x29_store(x29_add(A, Wt));
}

// W = 0 (n = 0): every row is the identity
static __global__ void __launch_bounds__(64) k_mb_close(const Xyzz<Fq>* __restrict__ wsums, MsmShape s, u32 rows, Fq* __restrict__ out_jac) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  X29 acc = x29_inf();
#pragma unroll 1
  for (u32 w = s.W; w-- > 0;) {
#pragma unroll 1
    for (u32 d = 0, nd = msm_width(s, w); d < nd; d++) acc = x29_dbl(acc);
    acc = x29_add(acc, x29_load(wsums[(size_t)j * s.W + w]));
  }
  store_norm_jac(out_jac + 3 * (size_t)j, x29_store(acc));
}

constexpr u32 QB_THREADS = 256;
// row = blockIdx.x: q[row * qstride + i - 1] = Q_i (1 <= i < n), values[row] = Q_0 with Q_i = c_i + z Q_(i+1); n >= 1
static __global__ void __launch_bounds__(QB_THREADS) k_fr_quotient_batch(const Fr* __restrict__ coeffs, u32 n, size_t stride, const Fr* __restrict__ points,
                                                                        Fr* __restrict__ q, size_t qstride, Fr* __restrict__ values) {
  __shared__ Fr h[QB_THREADS];
  const u32 t = threadIdx.x, L = (n + QB_THREADS - 1) / QB_THREADS;
  const size_t row = blockIdx.x;
  const Fr* __restrict__ c = coeffs + row * stride;
  const Fr z = points[row];
  const u32 lo = min(n, t * L), hi = min(n, lo + L);
  Fr acc = fp_zero<FrParams>();
#pragma unroll 1
  for (u32 k = hi; k-- > lo;) acc = fp_add<FrParams>(fp_mul<FrParams>(acc, z), c[k]);
  h[t] = acc;
  __syncthreads();
  if (t == 0) {
    Fr zl = fp_one<FrParams>(), b = z;                            // z^L
#pragma unroll 1
    for (u32 e = L; e; e >>= 1) {
      if (e & 1u) zl = fp_mul<FrParams>(zl, b);
      b = fp_mul<FrParams>(b, b);
    }
    Fr carry = fp_zero<FrParams>();                               // h[u] becomes the carry INTO segment u: Q at index (u + 1) L
#pragma unroll 1
    for (u32 u = QB_THREADS; u-- > 0;) {
      const Fr hu = h[u];
      h[u] = carry;
      carry = fp_add<FrParams>(fp_mul<FrParams>(carry, zl), hu);
    }
  }
  __syncthreads();
  acc = h[t];
#pragma unroll 1
  for (u32 k = hi; k-- > lo;) {
    acc = fp_add<FrParams>(fp_mul<FrParams>(acc, z), c[k]);
    if (k) q[row * qstride + k - 1] = acc;
    else if (values) values[row] = acc;
  }
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

static_assert(MB_N_MAX == N_BATCH_MAX, "internal.h names the limit of the batch kernels");

// window bits of the batch plan: about sixteen points per bucket, 256 slots per workgroup
int msm_batch_window(size_t n) {
  u32 c = MB_C_MIN;
  while (c < MB_C_MAX && (n >> (c - 1)) > 16) c++;
  return (int)c;
}
size_t msm_batch_rows_per_pass(size_t n, size_t m) {
  const size_t by_bytes = std::max<size_t>(1, MSM_BATCH_CANON_BYTES / (n * 32));
  return std::min(m, std::min<size_t>(by_bytes, MSM_BATCH_ROWS_MAX));
}

keaki_status msm_g1_batch_run(keaki_hip_ctx* ctx, const void* d_points, size_t srs_len, const void* d_table, int c_table, const void* d_scalars, size_t n,
                              size_t m, size_t stride, void* d_out_jac) {
  if (m == 0) return KEAKI_OK;
  hipStream_t st = ctx->stream;
  Fq* out = (Fq*)d_out_jac;
  if (n == 0) {
    MsmShape s = {0, 0, 0, 0, 0};
    for (size_t r0 = 0; r0 < m; r0 += (size_t)1 << 30) {
      const u32 rows = (u32)std::min<size_t>(m - r0, (size_t)1 << 30);
      hipLaunchKernelGGL(k_mb_close, dim3(cdiv(rows, 64)), dim3(64), 0, st, (const Xyzz<Fq>*)nullptr, s, rows, out + 3 * r0);
    }
    return launch_check(ctx, "mb_close");
  }
  bool batch = n <= N_BATCH_MAX;
  const MsmPlan plan = msm_make_plan(n, msm_batch_window(n));
  const size_t R = msm_batch_rows_per_pass(n, m);
  if (batch) {
    // optional memory, like the window tables: refused -> the rows go through the single-MSM pipeline instead of failing the call
    keaki_status ws = reserve(ctx, ctx->mb_canon, R * n * 32);
    if (ws == KEAKI_OK) ws = reserve(ctx, ctx->mb_wsums, R * plan.s.W * sizeof(Xyzz<Fq>));
    if (ws == KEAKI_ERR_OOM) { batch = false; ctx->err.clear(); }
    else if (ws != KEAKI_OK) return ws;
  }
  if (!batch) {
    for (size_t j = 0; j < m; j++)
      ST_TRY(msm_g1_run(ctx, d_points, srs_len, (const Fr*)d_scalars + j * stride, n, out + 3 * j, d_table, c_table, nullptr));
    return KEAKI_OK;
  }
  const MsmShape s = plan.s;
  const u32 c = s.c, logB = c - 1, G = MB_THREADS >> logB, groups = cdiv(s.W, G);
  MbBias bias = {};
  for (u32 w = 0; w + 1 < s.W; w++) {
    const u32 bit = (w < s.k ? (w + 1) * s.c : s.k * s.c + (w + 1 - s.k) * (s.c - 1)) - 1;      // offset(w) + width(w) - 1
    bias.l[bit >> 5] |= 1u << (bit & 31u);
  }
  for (size_t r0 = 0; r0 < m; r0 += R) {
    const u32 rows = (u32)std::min(R, m - r0);
    const u32 lanes = rows * (u32)n;
    hipLaunchKernelGGL(k_mb_canon, dim3(std::min<u32>(cdiv(lanes, 256), ctx->n_cu * 16u)), dim3(256), 0, st, (const Fr*)d_scalars + r0 * stride, (u32)n, rows,
                       stride, bias, (u32*)ctx->mb_canon.p);
    hipLaunchKernelGGL(k_mb_windows, dim3(groups, rows), dim3(MB_THREADS), 0, st, (const G1Aff*)d_points, (const u32*)ctx->mb_canon.p, s, logB,
                       (Xyzz<Fq>*)ctx->mb_wsums.p);
    hipLaunchKernelGGL(k_mb_close, dim3(cdiv(rows, 64)), dim3(64), 0, st, (const Xyzz<Fq>*)ctx->mb_wsums.p, s, rows, out + 3 * r0);
    ST_TRY(launch_check(ctx, "msm_batch"));
  }
  return KEAKI_OK;
}

keaki_status fr_quotient_batch_run(keaki_hip_ctx* ctx, const void* d_coeffs, size_t n, size_t m, size_t stride, const void* d_points, void* d_q, size_t qstride,
                                   void* d_values) {
  if (n == 0 || m == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_fr_quotient_batch, dim3((u32)m), dim3(QB_THREADS), 0, ctx->stream, (const Fr*)d_coeffs, (u32)n, stride, (const Fr*)d_points, (Fr*)d_q,
                     qstride, (Fr*)d_values);
  return launch_check(ctx, "fr_quotient_batch");
}

}  // namespace keaki_internal
