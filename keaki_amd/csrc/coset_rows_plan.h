// KZG coset pairs (kzg_coset_pairs.hip): the window table over the first l SRS points, the split of an item's l bases over lanes and the launch
// chunks. Host code only (no HIP), so that a plain C++ program can run it; tests/coset_pairs_model.py restates it and the CPU suite compares the two.
#pragma once
#include <cstdint>
#include <cstddef>

namespace keaki_internal {

// The table T[j][w][d] = d 2^(wb w) [tau^j]_1, j < l, holds l x windows x entries affine points of 64 B, in the layout of the fixed-base tables
// (ec_batch.hip.h: fb_shape): windows = ceil(254 / wb) (+ 1 when wb divides 254: the carry out of the top digit), entries = 2^(wb - 1) + 1 per window,
// slot 0 unused. A row costs l x windows mixed additions and no doublings.
//   wb   windows   bytes per base      additions per row
//   13      20      5,244,160          l = 4: 80     l = 64: 1,280
//   10      26        853,632          l = 128: 3,328   l = 512: 13,312
//    8      32        264,192          l = 1,024: 32,768
// The rule: the widest of 13 / 10 / 8 bits whose table stays at or under CR_TABLE_BYTES_MAX, 8 bits above that. MEASURED (profiles/coset_each_times.txt, the
// width sweep of bench_tools/bench_coset_each.py): the wider table won at every shape, also where it is far larger than the 256 MB Infinity Cache -- at
// d = 2^20 the call takes 4.19 / 3.48 / 3.02 ms at 8 / 10 / 13 bits for l = 64 (tables of 17 / 55 / 336 MB), 3.95 / 3.33 / 2.76 ms for l = 16 and
// 4.51 / 3.96 ms at 8 / 10 bits for l = 1,024 (270 / 874 MB). The first guess, a cap of 64 MiB (13 bits up to l = 8, 10 up to 64), lost 14 - 17 % there. The
// cap that ships is 512 MiB, a bound on what one handle may hold, not a cache size: 13 bits up to l = 64 (336 MB), 10 bits up to l = 512 (437 MB), 8 bits
// at l = 1,024 (270 MB; its 10-bit table of 874 MB was 12 % faster and is not the default).
constexpr size_t CR_TABLE_BYTES_MAX = (size_t)512 << 20;
constexpr uint32_t CR_WB_CANDIDATES[3] = {13, 10, 8};
inline uint32_t cr_windows(uint32_t wb) { return (254u + wb - 1u) / wb + ((254u % wb) == 0u ? 1u : 0u); }
inline uint32_t cr_entries(uint32_t wb) { return (1u << (wb - 1)) + 1u; }
inline size_t cr_table_bytes(uint32_t log2l, uint32_t wb) { return ((size_t)cr_windows(wb) * cr_entries(wb) << log2l) * 64; }
inline uint32_t cr_wb(uint32_t log2l) {
  for (uint32_t wb : CR_WB_CANDIDATES)
    if (cr_table_bytes(log2l, wb) <= CR_TABLE_BYTES_MAX) return wb;
  return 8;
}

// A launch of the row kernel with fewer lanes than this splits the l bases of an item over S neighbouring lanes of a wave (S a power of two, at most l
// and at most the 64 lanes of a wave): lane (k, s) sums the bases [s l / S, (s + 1) l / S) of item k. The constant is the threshold of the FK23 coset
// openings (fk_coset_plan.h: two resident waves on each of the 1,024 SIMDs); the option coset_rows_min_lanes replaces it. MEASURED (the same file, the lane
// sweep): at d = 2^20, l = 64 (16,384 items) 9.55 ms unsplit and at 2^14 lanes, 4.87 at 2^16, 3.11 at 2^17 and 2^18, 3.55 at 2^20; l = 1,024 (1,024 items):
// 220 ms unsplit, 15.0 at 2^14, 4.91 at 2^17, 4.71 at 2^20; l = 16: 2.72 at 2^17 against 2.71 at 2^18. 2^17 is within 4 % of the best everywhere.
constexpr uint32_t CR_MIN_LANES = 131072;
inline uint32_t cr_slices(uint64_t n, uint32_t log2l, uint64_t min_lanes_opt) {
  const uint64_t min_lanes = min_lanes_opt ? min_lanes_opt : CR_MIN_LANES;
  const uint32_t s_max = log2l < 6 ? 1u << log2l : 64u;
  uint32_t S = 1;
  while (n * S < min_lanes && S < s_max) S *= 2;
  return S;
}

// Items of a launch chunk: the scalar workspace holds the l rows of 32 B of every item of a chunk, about CR_CHUNK_VALUES values (32 MiB); an item at any
// l fits (l <= 1,024). A refused reservation halves the chunk (cr_chunk_halve), down to one item.
constexpr size_t CR_CHUNK_VALUES = (size_t)1 << 20;
inline size_t cr_chunk_items(size_t n, uint32_t log2l) {
  const size_t by_values = CR_CHUNK_VALUES >> log2l;
  return n < by_values ? n : by_values;
}
inline size_t cr_chunk_halve(size_t ch) { return (ch + 1) / 2; }

// route of a call: the option coset_rows_route (1 = the window table, 2 = the batched MSM over the rows), 0 = this plan. The table route is the plan's
// choice at every l -- MEASURED: it won at every shape, 2.6 - 3.6 x at d = 2^12, 3.2 - 13 x at 2^16, 2.6 - 62 x at 2^20 (the batched MSM is built for rows of
// thousands of scalars: 173 ms for 262,144 rows of 4) --; a refused table allocation falls back to route 2 whatever was asked for.
inline int cr_route(int route_opt, uint32_t /*log2l*/) { return route_opt == 2 ? 2 : 1; }

}  // namespace keaki_internal
