// KZG coset batch verification (keaki_hip_kzg_verify_cosets): the scalar-field side. Item k < n is a coset h_k <omega_l> of size l = 2^log2l with l
// claimed values y_(k,t) = p_k(h_k omega_l^t). Its interpolant is I_k(X) = sum_j a_(k,j) X^j with
//     a_(k,j) = h_k^-j b_(k,j),     b_k = the size-l inverse transform of y_k:  b_(k,j) = l^-1 sum_t y_(k,t) omega_l^(-j t)
// (I_k(h_k omega_l^t) = sum_j b_(k,j) omega_l^(j t) = y_(k,t)), and its vanishing polynomial is X^l - c_k, c_k = h_k^l. What the group side of the
// call (api.hip) needs from here:
//     -J_j = -sum_k gamma_k a_(k,j)  (j < l: the scalars of the MSM over [tau^j]_1)     s_k = gamma_k c_k  (the second MSM over the proofs)     g = sum gamma_k
//   k_vc_prepare    1 / h_k, s_k and the per-workgroup partial sums of g. A lane owns VC_INV = 16 consecutive items and inverts their shifts with ONE
//                   Fermat inversion (Montgomery's trick: prefix products up, one inversion, back down): 3 products + 1/16 of ~380 per item, so no
//                   l is too small for it. point_mode 1 (h_k = omega^k) runs the same code on the powers it steps through. A zero shift zeroes
//                   the prefix products behind it: the inverses of its 16 items come out 0 (the caller's contract, as repeated points for set_polys).
//   k_vc_transform  all inverse transforms in ONE launch. A workgroup takes tiles of T = VC_TILE_ELEMS / l items (1,024 values, 32 KB of LDS; an item
//                   at l = 1,024 is a tile), runs the log2 l butterfly stages of all T items side by side (decimation in frequency: natural order
//                   in, bit-reversed out; 512 butterflies a stage, two per lane, one product each, none in the last stage), then every lane takes
//                   four values in NATURAL order of j (one item's j0 .. j0 + 3 for l >= 4), multiplies them by gamma_k l^-1 h_k^-j and adds them to four
//                   registers that it keeps over all tiles of the workgroup: (l / 2) (log2 l - 1) + 2 l products per item, not l^2. h_k^-j0 comes
//                   from the item's table of squarings h_k^-(2^b) (LDS, log2 l entries, built by one lane per item), the next three by stepping. After
//                   its last tile the workgroup folds the T item slots (a tree in LDS) and writes ONE row of l partial sums.
//   k_vc_finish     folds the rows of all workgroups (any number of them, one pass: 64 values of j per workgroup, every fourth row per wave) and
//                   negates; workgroup 0 also folds g.
// Fr sums are exact: neither the tiling nor the number of workgroups changes a bit of the result.
// LDS layout: an Fr is 32 B. As an array of 32-byte structs a ds_read_b128 of 16 neighbouring lanes spans 512 B, two rows of the 64 banks: 2-way.
// Here a value lies in TWO planes of 16 B (words 0 - 3, words 4 - 7): neighbouring lanes read neighbouring 16-byte slots, 16 lanes = one bank row,
// conflict-free at unit stride (the butterflies of the last stages stride by 2, 4, ..: 2-way and up, against ~300 VALU instructions per product).
// Value e = slot * l + t of a tile sits at e + e / max(l, 16) (at most 64 slots of padding): in domain order neighbouring lanes load neighbouring
// ITEMS (see below), whose slots would otherwise be l values = a multiple of the bank row apart.
// Value addressing: (k, t) at values + 32 (k item_stride + t t_stride) bytes. When item_stride < t_stride (a vector in domain order: (1, r)) the lanes
// of a load run over the items of the tile first, so that one t of a tile is T x 32 contiguous bytes: whole 128-byte lines for l <= 256. At l =
// 512 / 1,024 a tile is 2 / 1 items and a line is shared by 2 / 4 tiles (neighbouring workgroups, through L2): every byte is still requested once.
// Otherwise (rows: (l, 1)) the lanes run over t first.
// One form for every l: a cross-lane form for items that fit a wave was not built -- at l <= 64 the call's time is the MSMs' (profiles/
// verify_cosets_times.txt has the transform kernel's own share), so there was nothing to win by it.
#include <algorithm>
#include <type_traits>
#include "internal.h"
#include "bn254_curve.hip.h"
#include "kzg_fr.hip.h"

namespace bn254 {

constexpr u32 VC_THREADS = 256, VC_WAVES = VC_THREADS / 64;
constexpr u32 VC_E = keaki_internal::VC_TILE_ELEMS;        // values of a tile
constexpr u32 VC_RUN = VC_E / VC_THREADS;                   // values a lane weighs and keeps: 4
constexpr u32 VC_INV = 16;                                  // items per Fermat inversion
constexpr u32 VC_AUX = 528;                                 // twiddles omega_l^-m (m < l / 2), then the squarings: l / 2 + T log2 l <= 522 for 2 <= l <= 1,024
static_assert(VC_E == 1024 && VC_RUN == 4, "the tile arithmetic below is written for 1,024 values on 256 lanes");

// The two 16-byte planes of a tile
struct VcTile {
  uint4 lo[VC_E + 64], hi[VC_E + 64];
};
KDEV u32 vc_phys(u32 e, u32 log2l) { return e + (e >> (log2l > 4u ? log2l : 4u)); }
KDEV Fr vc_ld(const VcTile& sh, u32 p) {
  const uint4 a = sh.lo[p], b = sh.hi[p];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
KDEV void vc_st(VcTile& sh, u32 p, const Fr& v) {
  sh.lo[p] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  sh.hi[p] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// f(0) .. f(K - 1) with a compile-time index
template <u32 K, class F>
KDEV void vc_each(F&& f) {
  if constexpr (K > 0) {
    vc_each<K - 1>(f);
    f(std::integral_constant<u32, K - 1>{});
  }
}

// Grid-stride over the chunks of VC_INV items. hinv_out and (point_mode 1) s_out double as the lane's own scratch on the way up.
// PAIRS (keaki_hip_kzg_coset_pairs: no gammas): s_out[k] = c_k itself, and nothing is summed.
template <int POINT_MODE, bool PAIRS = false>
static __global__ void __launch_bounds__(VC_THREADS) k_vc_prepare(const Fr* __restrict__ gammas, const Fr* __restrict__ points, u32 n, u32 log2l,
                                                                  Fr* __restrict__ s_out, Fr* __restrict__ hinv_out, Fr* __restrict__ part_g) {
  __shared__ Fr sh[VC_WAVES];
  const u32 chunks = (n + VC_INV - 1) / VC_INV, lanes = gridDim.x * VC_THREADS;
  Fr g = fp_zero<FrParams>();
  Fr omega = fp_zero<FrParams>();
  if constexpr (POINT_MODE == 1) omega = points[0];
#pragma unroll 1
  for (u32 c = blockIdx.x * VC_THREADS + threadIdx.x; c < chunks; c += lanes) {
    const u32 k0 = c * VC_INV, m = min(VC_INV, n - k0);
    Fr h = fp_zero<FrParams>(), pre = fp_one<FrParams>();
    if constexpr (POINT_MODE == 1) h = fr_pow_u32(omega, k0);
#pragma unroll 1
    for (u32 i = 0; i < m; i++) {                   // up: hinv_out[k] = h_k0 .. h_k
      if constexpr (POINT_MODE == 0) h = points[k0 + i];
      else s_out[k0 + i] = h;
      pre = fp_mul<FrParams>(pre, h);
      hinv_out[k0 + i] = pre;
      if constexpr (POINT_MODE == 1) h = fp_mul<FrParams>(h, omega);
    }
    Fr inv = fr_inv(pre);                           // 1 / (h_k0 .. h_(k0 + m - 1))
#pragma unroll 1
    for (u32 i = m; i-- > 0;) {                     // down
      const u32 k = k0 + i;
      if constexpr (POINT_MODE == 0) h = points[k];
      else h = s_out[k];
      hinv_out[k] = i ? fp_mul<FrParams>(inv, hinv_out[k - 1]) : inv;
      inv = fp_mul<FrParams>(inv, h);
      Fr ck = h;                                    // c_k = h_k^l
#pragma unroll 1
      for (u32 b = 0; b < log2l; b++) ck = fp_mul<FrParams>(ck, ck);
      if constexpr (PAIRS) {
        s_out[k] = ck;
      } else {
        const Fr gamma = gammas[k];
        s_out[k] = fp_mul<FrParams>(gamma, ck);
        g = fp_add<FrParams>(g, gamma);
      }
    }
  }
  if constexpr (PAIRS) return;
  g = fr_wave_sum(g);
  if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (u32 w = 1; w < VC_WAVES; w++) g = fp_add<FrParams>(g, sh[w]);
    part_g[blockIdx.x] = g;
  }
}

// part_j[blockIdx.x * l + j] = sum over the items k of this workgroup's tiles of gamma_k l^-1 h_k^-j b'_(k,j), b' the transform without its l^-1.
// BY_ITEM: the lanes of a load run over the items of the tile first (item_stride < t_stride).
// ROWS (keaki_hip_kzg_coset_pairs): no gammas and no sum over the items -- every item's row is stored: rows_out[k * l + j] = -a_(k,j) = -l^-1 h_k^-j b'_(k,j),
// 32 B each, as a canonical integer (rows_mont = 0: the digits of the window-table walk) or in Montgomery form (1: the scalars of the batched MSM).
template <bool BY_ITEM, bool ROWS = false>
static __global__ void __launch_bounds__(VC_THREADS) k_vc_transform(const Fr* __restrict__ values, u64 item_stride, u64 t_stride, const Fr* __restrict__ gammas,
                                                                    const Fr* __restrict__ hinv, Fr omega_l_inv, Fr inv_l, u32 log2l, u32 n,
                                                                    Fr* __restrict__ part_j, u32* __restrict__ rows_out = nullptr, u32 rows_mont = 0) {
  __shared__ VcTile sh;
  __shared__ Fr aux[VC_AUX];
  const u32 tid = threadIdx.x;
  const u32 l = 1u << log2l, half_l = l >> 1;
  const u32 log2T = 10u - log2l, T = 1u << log2T;
  Fr* const tw = aux;
  Fr* const sq = aux + half_l;                      // sq[slot * log2l + b] = h_k^-(2^b)
  const u32 tiles = (n + T - 1) >> log2T;
  for (u32 m = tid; m < half_l; m += VC_THREADS) tw[m] = fr_pow_u32(omega_l_inv, m);
  Fr acc[VC_RUN];
#pragma unroll
  for (u32 i = 0; i < VC_RUN; i++) acc[i] = fp_zero<FrParams>();

#pragma unroll 1
  for (u32 q = blockIdx.x; q < tiles; q += gridDim.x) {
    const u32 k_base = q << log2T;
    // the tile's values (zeros for the slots past n) and its squarings
#pragma unroll
    for (u32 i = 0; i < VC_RUN; i++) {
      const u32 idx = tid + VC_THREADS * i;
      const u32 slot = BY_ITEM ? (idx & (T - 1)) : (idx >> log2l), t = BY_ITEM ? (idx >> log2T) : (idx & (l - 1));
      const u32 k = k_base + slot;
      const Fr v = k < n ? values[(u64)k * item_stride + (u64)t * t_stride] : fp_zero<FrParams>();
      vc_st(sh, vc_phys((slot << log2l) + t, log2l), v);
    }
    if (log2l)
      for (u32 slot = tid; slot < T; slot += VC_THREADS) {
        const u32 k = k_base + slot;
        Fr x = k < n ? hinv[k] : fp_zero<FrParams>();
#pragma unroll 1
        for (u32 b = 0; b < log2l; b++) {
          sq[slot * log2l + b] = x;
          x = fp_mul<FrParams>(x, x);
        }
      }
    __syncthreads();
    // decimation in frequency: stage s pairs i0 and i0 + 2^s with the twiddle omega_l^-(off 2^(log2l - 1 - s))
#pragma unroll 1
    for (u32 s = log2l; s-- > 0;) {
      const u32 half = 1u << s;
#pragma unroll
      for (u32 i = 0; i < VC_E / 2 / VC_THREADS; i++) {
        const u32 b = tid + VC_THREADS * i;
        const u32 slot = b >> (log2l - 1), r = b & (half_l - 1);
        const u32 off = r & (half - 1), i0 = ((r >> s) << (s + 1)) + off;
        const u32 p0 = vc_phys((slot << log2l) + i0, log2l), p1 = vc_phys((slot << log2l) + i0 + half, log2l);
        const Fr u = vc_ld(sh, p0), v = vc_ld(sh, p1);
        vc_st(sh, p0, fp_add<FrParams>(u, v));
        Fr d = fp_sub<FrParams>(u, v);
        if (s) d = fp_mul<FrParams>(d, tw[off << (log2l - 1 - s)]);
        vc_st(sh, p1, d);
      }
      __syncthreads();
    }
    // weigh: value e = 4 tid + i in natural order of j; position brev(j) of its item holds it
    Fr pw = fp_zero<FrParams>();
    vc_each<VC_RUN>([&](auto ic) {                  // compile-time i: acc[] stays in registers (a plain unrolled loop left it in scratch memory)
      constexpr u32 i = decltype(ic)::value;
      const u32 e = VC_RUN * tid + i;
      const u32 slot = e >> log2l, j = e & (l - 1);
      const u32 k = k_base + slot;
      if (k < n) {
        if (i == 0 || j == 0) {
          if constexpr (ROWS) pw = inv_l;
          else pw = fp_mul<FrParams>(gammas[k], inv_l);
#pragma unroll 1
          for (u32 b = 0; b < log2l; b++)
            if ((j >> b) & 1u) pw = fp_mul<FrParams>(pw, sq[slot * log2l + b]);
        } else {
          pw = fp_mul<FrParams>(pw, sq[slot * log2l]);
        }
        const u32 p = log2l ? (__brev(j) >> (32u - log2l)) : 0u;
        const Fr term = fp_mul<FrParams>(vc_ld(sh, vc_phys((slot << log2l) + p, log2l)), pw);
        if constexpr (ROWS) {
          const Fr na = fp_neg<FrParams>(term);
          u32 v[8];
          if (rows_mont) {
#pragma unroll
            for (int w = 0; w < 8; w++) v[w] = na.l[w];
          } else {
            fp_from_mont<FrParams>(v, na);
          }
          uint4* dst = reinterpret_cast<uint4*>(rows_out + (((size_t)k << log2l) + j) * 8u);
          dst[0] = make_uint4(v[0], v[1], v[2], v[3]);
          dst[1] = make_uint4(v[4], v[5], v[6], v[7]);
        } else {
          acc[i] = fp_add<FrParams>(acc[i], term);
        }
      }
    });
    __syncthreads();                                // the next tile overwrites the values and the squarings
  }

  if constexpr (ROWS) return;
  // fold the T slots: value e = slot * l + j (natural order now), a tree over the slots
  vc_each<VC_RUN>([&](auto ic) { vc_st(sh, vc_phys(VC_RUN * tid + decltype(ic)::value, log2l), acc[decltype(ic)::value]); });
  __syncthreads();
#pragma unroll 1
  for (u32 h = VC_E / 2; h >= l; h >>= 1) {
    for (u32 e = tid; e < h; e += VC_THREADS) {
      const u32 p = vc_phys(e, log2l);
      vc_st(sh, p, fp_add<FrParams>(vc_ld(sh, p), vc_ld(sh, vc_phys(e + h, log2l))));
    }
    __syncthreads();
  }
  for (u32 j = tid; j < l; j += VC_THREADS) part_j[(size_t)blockIdx.x * l + j] = vc_ld(sh, vc_phys(j, log2l));
}

// neg_j[j] = -sum over the `blocks` rows of part_j: a workgroup takes 64 values of j, its four waves every fourth row each (the loads of a wave are
// 2 KB of one row; with ONE lane per j running over all rows the kernel took 0.28 ms at 768 rows, all of it load latency), then LDS folds the four.
// Workgroup 0: g_out = the sum of the g_blocks entries of part_g.
static __global__ void __launch_bounds__(VC_THREADS) k_vc_finish(const Fr* __restrict__ part_j, u32 blocks, u32 l, const Fr* __restrict__ part_g, u32 g_blocks,
                                                                 Fr* __restrict__ neg_j, Fr* __restrict__ g_out) {
  __shared__ Fr sh[VC_THREADS];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u32 j = blockIdx.x * 64u + lane;
  Fr sum = fp_zero<FrParams>();
  if (j < l) {
#pragma unroll 4
    for (u32 b = wave; b < blocks; b += VC_WAVES) sum = fp_add<FrParams>(sum, part_j[(size_t)b * l + j]);
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  if (wave == 0 && j < l) {
#pragma unroll
    for (u32 w = 1; w < VC_WAVES; w++) sum = fp_add<FrParams>(sum, sh[w * 64u + lane]);
    neg_j[j] = fp_neg<FrParams>(sum);
  }
  if (blockIdx.x) return;                           // uniform per workgroup
  __syncthreads();                                  // sh is free again
  Fr g = fp_zero<FrParams>();
#pragma unroll 1
  for (u32 b = threadIdx.x; b < g_blocks; b += VC_THREADS) g = fp_add<FrParams>(g, part_g[b]);
  g = fr_wave_sum(g);
  if (lane == 0) sh[wave] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (u32 w = 1; w < VC_WAVES; w++) g = fp_add<FrParams>(g, sh[w]);
    *g_out = g;
  }
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

namespace {
constexpr u32 VC_G_BLOCKS = 1024;            // most workgroups of k_vc_prepare = entries of part_g
u32 vc_tiles(size_t n, uint32_t log2l) { return cdiv(n, VC_TILE_ELEMS >> log2l); }
u32 vc_rows_max(size_t n, uint32_t log2l) { return std::min<u32>(vc_tiles(n, log2l), VC_MAX_BLOCKS); }
}  // namespace

// [s: n | 1 / h: n | -J: l | g: 1 | part_g: VC_G_BLOCKS | part_j: rows x l] Fr
size_t verify_cosets_work_bytes(size_t n, uint32_t log2l) {
  return (2 * n + ((size_t)1 << log2l) + 1 + VC_G_BLOCKS + ((size_t)vc_rows_max(n, log2l) << log2l)) * sizeof(Fr);
}
VcWork verify_cosets_layout(size_t n, uint32_t log2l, void* d_work) {
  Fr* p = (Fr*)d_work;
  VcWork w;
  w.s = p; p += n;
  w.hinv = p; p += n;
  w.neg_j = p; p += (size_t)1 << log2l;
  w.g = p; p += 1;
  w.part_g = p; p += VC_G_BLOCKS;
  w.part_j = p;
  return w;
}

keaki_status verify_cosets_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const void* d_values, size_t item_stride,
                                       size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, const VcWork& w) {
  if (n == 0 || log2l > 10 || ((size_t)1 << log2l) > KEAKI_SET_MAX || (n << log2l) >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_verify_cosets: n = %zu items of 2^%u values out of range on the device side", n, log2l);
  const u32 l = 1u << log2l;
  Fr winv, linv;
  memcpy(&winv, omega_l_inv, 32);
  memcpy(&linv, inv_l, 32);
  const u32 g_blocks = std::min<u32>(cdiv(cdiv(n, VC_INV), VC_THREADS), VC_G_BLOCKS);
  if (point_mode)
    hipLaunchKernelGGL(k_vc_prepare<1>, dim3(g_blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)d_gammas, (const Fr*)d_points, (u32)n, log2l, (Fr*)w.s,
                       (Fr*)w.hinv, (Fr*)w.part_g);
  else
    hipLaunchKernelGGL(k_vc_prepare<0>, dim3(g_blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)d_gammas, (const Fr*)d_points, (u32)n, log2l, (Fr*)w.s,
                       (Fr*)w.hinv, (Fr*)w.part_g);
  // three workgroups of 50.5 KB fit a compute unit's LDS; the rows the workspace holds bound the grid
  const int opt = ctx->tune.verify_cosets_blocks;
  const u32 cap = opt > 0 ? (u32)opt : ctx->n_cu * 3u;
  const u32 blocks = std::min<u32>(vc_rows_max(n, log2l), cap);
  if (item_stride < t_stride)
    hipLaunchKernelGGL(k_vc_transform<true>, dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)d_values, (u64)item_stride, (u64)t_stride,
                       (const Fr*)d_gammas, (const Fr*)w.hinv, winv, linv, log2l, (u32)n, (Fr*)w.part_j);
  else
    hipLaunchKernelGGL(k_vc_transform<false>, dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)d_values, (u64)item_stride, (u64)t_stride,
                       (const Fr*)d_gammas, (const Fr*)w.hinv, winv, linv, log2l, (u32)n, (Fr*)w.part_j);
  hipLaunchKernelGGL(k_vc_finish, dim3(cdiv(l, 64)), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)w.part_j, blocks, l, (const Fr*)w.part_g, g_blocks,
                     (Fr*)w.neg_j, (Fr*)w.g);
  return launch_check(ctx, "verify_cosets_scalars");
}

// keaki_hip_kzg_coset_pairs, Fr side. coset_pairs_shifts_run: d_c_out[k] = c_k = h_k^l (Montgomery) and d_hinv[k] = 1 / h_k for ALL n items of the call
// (point_mode 1 steps through omega^k from k = 0). coset_pairs_rows_run: the rows -a_(k,j) of the m items from `first` on into d_rows (m x l x 32 B, in
// (item, j) order; mont: see k_vc_transform), one launch.
keaki_status coset_pairs_shifts_run(keaki_hip_ctx* ctx, const void* d_points, int point_mode, uint32_t log2l, size_t n, void* d_c_out, void* d_hinv) {
  if (n == 0 || n >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_coset_pairs: n = %zu out of range on the device side", n);
  const u32 blocks = std::min<u32>(cdiv(cdiv(n, VC_INV), VC_THREADS), VC_G_BLOCKS);
  if (point_mode)
    hipLaunchKernelGGL((k_vc_prepare<1, true>), dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)nullptr, (const Fr*)d_points, (u32)n, log2l,
                       (Fr*)d_c_out, (Fr*)d_hinv, (Fr*)nullptr);
  else
    hipLaunchKernelGGL((k_vc_prepare<0, true>), dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, (const Fr*)nullptr, (const Fr*)d_points, (u32)n, log2l,
                       (Fr*)d_c_out, (Fr*)d_hinv, (Fr*)nullptr);
  return launch_check(ctx, "coset_pairs_shifts");
}
keaki_status coset_pairs_rows_run(keaki_hip_ctx* ctx, const void* d_values, size_t item_stride, size_t t_stride, const void* d_hinv, uint32_t log2l,
                                  const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t first, size_t m, bool mont, void* d_rows) {
  if (m == 0 || log2l > 10 || ((size_t)1 << log2l) > KEAKI_SET_MAX || (m << log2l) >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_coset_pairs: a chunk of %zu items of 2^%u values out of range on the device side", m, log2l);
  Fr winv, linv;
  memcpy(&winv, omega_l_inv, 32);
  memcpy(&linv, inv_l, 32);
  const Fr* values = (const Fr*)d_values + first * item_stride;
  const Fr* hinv = (const Fr*)d_hinv + first;
  const u32 blocks = std::min<u32>(vc_tiles(m, log2l), ctx->n_cu * 3u);
  if (item_stride < t_stride)
    hipLaunchKernelGGL((k_vc_transform<true, true>), dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, values, (u64)item_stride, (u64)t_stride, (const Fr*)nullptr,
                       hinv, winv, linv, log2l, (u32)m, (Fr*)nullptr, (u32*)d_rows, mont ? 1u : 0u);
  else
    hipLaunchKernelGGL((k_vc_transform<false, true>), dim3(blocks), dim3(VC_THREADS), 0, ctx->stream, values, (u64)item_stride, (u64)t_stride, (const Fr*)nullptr,
                       hinv, winv, linv, log2l, (u32)m, (Fr*)nullptr, (u32*)d_rows, mont ? 1u : 0u);
  return launch_check(ctx, "coset_pairs_rows");
}

}  // namespace keaki_internal
