// FK23 coset openings (fk_coset.hip): how the host cuts the l terms of a position over lanes and groups. Host code only (no HIP), so that a
// plain C++ program can run it; tests/fk_coset_model.py restates it (split_plan) and the CPU suite compares the two texts' constants.
#pragma once
#include <cstdint>

namespace keaki_internal {

// terms of one Straus group: G window tables (1 KB each per lane) share one chain of 129 doublings
constexpr uint32_t FKC_G = 4;
// A launch of the pointwise kernel with fewer lanes than this splits the l terms of a position over S lanes. MEASURED (profiles/fk_coset_times.txt,
// the threshold sweep of bench_tools/bench_fk_coset.py): 131,072 lanes are the kernel's two resident waves on each of the 1,024 SIMDs. At d = 2^20,
// l = 64 (2^15 positions) the kernel takes 31.3 ms unsplit, 28.6 ms at 2^16 lanes, 17.5 ms at 2^17 and 17.1 / 16.7 ms at 2^18 / 2^19; at l = 16 (2^17
// positions) 17.0 unsplit against 16.6 / 16.2 at 2^18 / 2^19 lanes: beyond one full residency a further split buys 2 - 5 % for twice the tables.
// (The first guess was 65,536, one wave per SIMD.)
constexpr uint32_t FKC_SPLIT_MIN_LANES = 131072;

struct FkcPlan {
  uint32_t G;        // terms per group: min(g, l), g in {1, 2, 4}
  uint32_t S;        // lanes per position (a power of two): lane (s, q) sums the terms [s l / S, (s + 1) l / S) of position q
  uint32_t groups;   // groups per lane: l / (S G)
};
// n2 = 2r positions of l = 2^log2l terms each. g_opt / min_lanes_opt: the options fk_coset_group / fk_coset_min_lanes, 0 = the constants above.
// S doubles while the launch stays below min_lanes and every lane keeps at least one full group.
inline FkcPlan fkc_plan(uint64_t n2, uint32_t l, uint32_t g_opt, uint64_t min_lanes_opt) {
  FkcPlan p;
  p.G = g_opt ? g_opt : FKC_G;
  if (p.G > l) p.G = l;
  const uint64_t min_lanes = min_lanes_opt ? min_lanes_opt : FKC_SPLIT_MIN_LANES;
  p.S = 1;
  while (n2 * p.S < min_lanes && l / (2 * p.S) >= p.G) p.S *= 2;
  p.groups = l / (p.S * p.G);
  return p;
}

}  // namespace keaki_internal
