// How encap_multi / encrypt_multi read their group offsets and split the groups between the two routes: integer work on the offsets and
// the option "encap_multi_single_min" alone. No HIP call and no HIP header, so keaki_amd/host/encap_multi_plan_main.cpp checks the
// invariants on a CPU (tests/test_encap_multi_plan_cpu.py), and the library (api.hip) runs the same code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace keaki_internal {

// Group j of a call is items [offsets[j], offsets[j + 1]), j < m: the array starts at 0, never decreases and ends at n < 2^31 (the
// kernels index items, and groups, with 32 bits: m < 2^31 too). Empty groups are allowed anywhere; m = 0 needs n = 0.
inline bool encap_multi_offsets_ok(const uint64_t* offsets, size_t m, size_t n) {
  if (!offsets || n >= ((size_t)1 << 31) || m >= ((size_t)1 << 31) || offsets[0] != 0) return false;
  for (size_t j = 0; j < m; j++)
    if (offsets[j + 1] < offsets[j]) return false;
  return offsets[m] == (uint64_t)n;
}

// A piece of a call: groups [g_lo, g_hi) = items [i_lo, i_hi). single: ONE group of at least single_min items, for the single-commitment
// path (GT tables); else a maximal run of consecutive smaller groups, for the fused route (a pairing per item). A run may hold no item.
struct EncapMultiPiece {
  size_t g_lo, g_hi, i_lo, i_hi;
  bool single;
};
// The pieces in order: their group ranges partition [0, m), their item ranges [0, n). single_min <= 0: never the single path.
// `offsets` has passed encap_multi_offsets_ok.
inline std::vector<EncapMultiPiece> encap_multi_plan(const uint64_t* offsets, size_t m, long long single_min) {
  std::vector<EncapMultiPiece> pieces;
  size_t run_lo = 0;
  for (size_t j = 0; j < m; j++) {
    const uint64_t k = offsets[j + 1] - offsets[j];
    if (single_min <= 0 || k < (uint64_t)single_min) continue;
    if (j > run_lo) pieces.push_back({run_lo, j, (size_t)offsets[run_lo], (size_t)offsets[j], false});
    pieces.push_back({j, j + 1, (size_t)offsets[j], (size_t)offsets[j + 1], true});
    run_lo = j + 1;
  }
  if (m > run_lo) pieces.push_back({run_lo, m, (size_t)offsets[run_lo], (size_t)offsets[m], false});
  return pieces;
}

}  // namespace keaki_internal
