// KZG set pairs (kzg_set_pairs.hip): the window table over the first kb G2 points of the SRS, the split of an item's bases over lanes and the launch
// chunks. Host code only (no HIP), so that a plain C++ program can run it; tests/set_pairs_model.py restates it and the CPU suite compares the two.
#pragma once
#include <cstdint>
#include <cstddef>

namespace keaki_internal {

// The table T2[j][w][d] = d 2^(wb w) [tau^j]_2, j < kb, holds kb x windows x entries affine G2 points of 128 B, in the layout of the fixed-base tables
// (ec_batch.hip.h: fb_shape): windows = ceil(254 / wb) (+ 1 when wb divides 254: the carry out of the top digit), entries = 2^(wb - 1) + 1 per window,
// slot 0 unused. It is base-major: the table of kb bases is a prefix of the table of any more, so it serves every k <= kb. A row costs k x windows mixed
// additions and no doublings.
//   wb   windows   bytes per base      additions per row
//   13      20     10,488,320          k = 2: 40      k = 8: 160     k = 64: 1,280
//   10      26      1,707,264          k = 2: 52      k = 8: 208     k = 64: 1,664
//    8      32        528,384          k = 2: 64      k = 8: 256     k = 64: 2,048
// The rule is the coset table's (coset_rows_plan.h): the widest of 13 / 10 / 8 bits whose table stays at or under SR_TABLE_BYTES_MAX, a bound on what one
// handle may hold: 13 bits up to k = 51 (535 MB), 10 bits up to k = 64 (109 MB). MEASURED (profiles/set_each_times.txt, the width sweep of
// bench_tools/bench_set_each.py, set_pairs resident): the wider table won at every shape -- n = 2^16: k = 2 1.97 / 1.76 / 1.57 ms at 8 / 10 / 13 bits (tables
// of 1.1 / 3.4 / 21 MB), k = 8 5.47 / 4.72 / 4.16 ms (4.2 / 13.7 / 84 MB), k = 64 59.4 / 54.6 ms at 8 / 10 bits (34 / 109 MB); n = 4,096: 1.28 / 1.21 / 1.13,
// 1.53 / 1.46 / 1.37 and 5.39 / 5.07 ms. The 13-bit table of k > 51 (671 MB at k = 64) is over the cap and was NOT measured. The build of a first call:
// 3.2 - 7.8 ms (k = 2 at 8 bits .. k = 8 at 13 bits 7.7 ms, k = 64 at 10 bits 7.8 ms).
constexpr size_t SR_TABLE_BYTES_MAX = (size_t)512 << 20;
constexpr uint32_t SR_WB_CANDIDATES[3] = {13, 10, 8};
inline uint32_t sr_windows(uint32_t wb) { return (254u + wb - 1u) / wb + ((254u % wb) == 0u ? 1u : 0u); }
inline uint32_t sr_entries(uint32_t wb) { return (1u << (wb - 1)) + 1u; }
inline size_t sr_table_bytes(size_t kb, uint32_t wb) { return (size_t)sr_windows(wb) * sr_entries(wb) * kb * 128; }
inline uint32_t sr_wb(size_t kb) {
  for (uint32_t wb : SR_WB_CANDIDATES)
    if (sr_table_bytes(kb, wb) <= SR_TABLE_BYTES_MAX) return wb;
  return 8;
}
// the width a refused table falls to: 13 -> 10 -> 8 -> 0 (none left: KEAKI_ERR_OOM)
inline uint32_t sr_wb_narrower(uint32_t wb) { return wb > 10 ? 10u : wb > 8 ? 8u : 0u; }

inline uint32_t sr_log2kp(size_t k) { uint32_t b = 0; while (((size_t)1 << b) < k) b++; return b; }

// A launch of the G2 row kernel with fewer lanes than this splits the kp = 2^log2kp base slots of an item (the k bases and the padding) over S neighbouring
// lanes of a wave (S a power of two, at most kp and at most 64): lane (i, s) sums the bases [s kp / S, (s + 1) kp / S) below k of item i. The constant
// is half the coset rows' (coset_rows_plan.h: 2^17). MEASURED (the same file, the lane sweep, set_pairs resident, ms at 1 (never split) /
// 2^14 / 2^16 / 2^17 / 2^18 / 2^20 lanes): n = 64, k = 64: 23.3 / 2.96 / 2.96 / 2.95 / 2.96 / 2.95; n = 4,096, k = 8: 3.64 / 1.74 / 1.45 / 1.44 / 1.45 / 1.45;
// n = 4,096, k = 64: 24.6 / 8.96 / 5.13 / 5.38 / 5.65 / 5.66; n = 2^16, k = 8: 4.68 / 4.67 / 4.67 / 5.19 / 5.38 / 5.78. 2^16 is the best or within 1 % of it at
// all four; 2^17 loses 5 % and 11 % at the last two (a G2 addition is long enough that one wave per SIMD already hides the table loads, and a split pays
// general additions for the exchange). The option set_rows_min_lanes replaces it.
constexpr uint32_t SR_MIN_LANES = 65536;
inline uint32_t sr_slices(uint64_t n, uint32_t log2kp, uint64_t min_lanes_opt) {
  const uint64_t min_lanes = min_lanes_opt ? min_lanes_opt : SR_MIN_LANES;
  const uint32_t s_max = log2kp < 6 ? 1u << log2kp : 64u;
  uint32_t S = 1;
  while (n * S < min_lanes && S < s_max) S *= 2;
  return S;
}

// Items of a launch chunk of set_pairs: the scalar workspace holds the kp + 2 k (+ k) values of 32 B of every item of a chunk, about SR_CHUNK_VALUES padded
// values (32 MiB of -I rows); an item at any k fits. A refused reservation halves the chunk (sr_chunk_halve), down to one item.
constexpr size_t SR_CHUNK_VALUES = (size_t)1 << 20;
inline size_t sr_chunk_items(size_t n, uint32_t log2kp) {
  const size_t by_values = SR_CHUNK_VALUES >> log2kp;
  return n < by_values ? n : by_values;
}
inline size_t sr_chunk_halve(size_t ch) { return (ch + 1) / 2; }
// bytes of that workspace per item: [w: k | pts: k (point_mode 1) | rows_i: kp | rows_z: k] Fr, [G1 XYZZ 128] [G2 XYZZ 256] [G1 Jacobian 96 (MSM route)]
inline size_t sr_item_bytes(size_t k, uint32_t log2kp, int point_mode, bool msm_route) {
  return (((size_t)1 << log2kp) + (point_mode ? 3 : 2) * k) * 32 + 128 + 256 + (msm_route ? 96 : 0);
}

// How verify_sets_each decides its items: the option set_each_route (1 = the fused kernel k_pairing2v, 2 = two Miller loops per item through the existing
// kernels, a pairwise GT product, the final exponentiation, a comparison), 0 = this plan. The plan is route 2 at every n -- MEASURED (the same file; k = 2,
// resident, route 1 / route 2 in ms): n = 2 6.8 / 2.5, 64 7.1 / 2.7, 4,096 7.1 / 4.8, 8,192 7.1 / 6.4, 16,384 7.2 / 6.6, 32,768 7.4 / 8.5, 65,536 18.3 / 16.4,
// 2^17 36.5 / 30.9, 2^18 74.4 / 59.5, 2^20 300 / 230. The fused kernel saves the second chain of squarings but computes the lines of Z2_i in a lane pair
// that also carries f (one pairing's latency, ~6 ms, is its floor at any n); the two-loop route runs small batches on the twelve-lane kernels and large ones
// at k_pairing's own rate. The fused kernel won only at n = 32,768 (by 13 %); it ships as the A/B form.
inline int se_route(int route_opt, size_t /*n*/) { return route_opt == 1 ? 1 : 2; }

// Items of a launch chunk of verify_sets_each's pairing side: route 2 runs 2 m Miller loops in one launch, so half of what a pairing launch takes; a refused
// reservation halves it down to SE_CHUNK_MIN (one wave of lane pairs), as verify_each does.
constexpr size_t SE_CHUNK_MIN = 32;
inline size_t se_chunk_items(size_t n, size_t pairing_launch_items) {
  const size_t cap = pairing_launch_items / 2;
  return n < cap ? n : cap;
}
inline size_t se_chunk_halve(size_t ch) {
  const size_t h = ((ch + 1) / 2 + 31) & ~(size_t)31;
  return h < SE_CHUNK_MIN ? SE_CHUNK_MIN : h;
}
// bytes per item of that chunk: route 2 [ps: 2 x 64] [qs: 2 x 128] [miller: 2 x 384] [product 384] [gt 384]; the fused kernel needs [-proof 64] only
inline size_t se_item_bytes(bool route2) { return route2 ? 128 + 256 + 768 + 384 + 384 : 64; }

}  // namespace keaki_internal
