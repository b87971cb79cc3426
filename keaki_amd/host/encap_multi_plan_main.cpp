// The group offsets of encap_multi / encrypt_multi (keaki_amd/csrc/encap_multi_plan.h: encap_multi_offsets_ok, encap_multi_plan) on a CPU,
// under AddressSanitizer / UBSan (make encap_multi_plan_asan; tests/test_encap_multi_plan_cpu.py): over random and adversarial offset arrays
// and thresholds the pieces partition the groups and the items in order, single pieces are exactly the groups at or above the threshold,
// every bad array is refused, and the item-to-group search of k_encap_multi_g1 (kem_multi.hip), restated below, finds for every item the
// group that holds it -- over the whole array and over each fused run's sub-array, the form the library hands the kernel.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/encap_multi_plan.h"

using namespace keaki_internal;

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                            \
  } while (0)

// the search of k_encap_multi_g1, word for word: offsets holds m + 1 words, offsets[0] <= gi < offsets[m]
static uint32_t group_of(const uint64_t* offsets, uint32_t m, uint64_t gi) {
  uint32_t lo = 0, hi = m;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= gi) lo = mid; else hi = mid;
  }
  return lo;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {            // SplitMix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static size_t arrays = 0, searched = 0;

// `full`: search every item (else the first and last item of every group)
static void check_sizes(const std::vector<uint64_t>& sizes, const char* what, bool full = true) {
  const size_t m = sizes.size();
  std::vector<uint64_t> off(m + 1, 0);           // exactly m + 1 words: a read past either end is the sanitizer's
  for (size_t j = 0; j < m; j++) off[j + 1] = off[j] + sizes[j];
  const size_t n = (size_t)off[m];
  arrays++;
  CHECK(encap_multi_offsets_ok(off.data(), m, n), "%s: m %zu n %zu refused", what, m, n);
  CHECK(!encap_multi_offsets_ok(off.data(), m, n + 1), "%s: wrong n accepted", what);
  if (n) CHECK(!encap_multi_offsets_ok(off.data(), m, n - 1), "%s: wrong n accepted", what);
  uint64_t biggest = 0;
  for (uint64_t k : sizes) if (k > biggest) biggest = k;
  std::vector<long long> thresholds = {0, 1, 2, 64, 8192, -1};
  for (size_t j = 0; j < m && j < 4; j++) { thresholds.push_back((long long)sizes[j]); thresholds.push_back((long long)sizes[j] + 1); }
  thresholds.push_back((long long)biggest); thresholds.push_back((long long)biggest + 1);
  for (long long t : thresholds) {
    const std::vector<EncapMultiPiece> pieces = encap_multi_plan(off.data(), m, t);
    size_t g = 0, i = 0;
    bool last_run = false;
    for (size_t q = 0; q < pieces.size(); q++) {
      const EncapMultiPiece& p = pieces[q];
      CHECK(p.g_lo == g && p.g_hi > p.g_lo && p.g_hi <= m, "%s t %lld: piece %zu groups [%zu, %zu) after %zu", what, t, q, p.g_lo, p.g_hi, g);
      CHECK(p.i_lo == i && p.i_lo == off[p.g_lo] && p.i_hi == off[p.g_hi], "%s t %lld: piece %zu items [%zu, %zu) after %zu", what, t, q, p.i_lo, p.i_hi, i);
      if (p.g_hi <= p.g_lo || p.g_hi > m) return;
      if (p.single) {
        CHECK(p.g_hi == p.g_lo + 1 && t > 0 && sizes[p.g_lo] >= (uint64_t)t, "%s t %lld: single piece %zu", what, t, q);
      } else {
        CHECK(!last_run || q == 0, "%s t %lld: run %zu follows a run (not maximal)", what, t, q);
        for (size_t j = p.g_lo; j < p.g_hi; j++) CHECK(t <= 0 || sizes[j] < (uint64_t)t, "%s t %lld: group %zu of %llu items in a run", what, t, j, (unsigned long long)sizes[j]);
        // the kernel searches the run's own offsets with the item's GLOBAL index
        for (size_t j = p.g_lo; j < p.g_hi; j++)
          for (uint64_t x = off[j]; x < off[j + 1]; x = (full || x + 1 == off[j + 1]) ? x + 1 : off[j + 1] - 1) {
            const uint32_t got = group_of(off.data() + p.g_lo, (uint32_t)(p.g_hi - p.g_lo), x);
            CHECK(p.g_lo + got == j, "%s t %lld: item %llu of group %zu found in %zu", what, t, (unsigned long long)x, j, p.g_lo + got);
            searched++;
          }
      }
      last_run = !p.single;
      g = p.g_hi; i = p.i_hi;
    }
    CHECK(g == m && i == n, "%s t %lld: pieces end at group %zu of %zu, item %zu of %zu", what, t, g, m, i, n);
  }
  // the search over the whole array: the j with off[j] <= x < off[j + 1]
  for (size_t j = 0; j < m; j++)
    for (uint64_t x = off[j]; x < off[j + 1]; x = (full || x + 1 == off[j + 1]) ? x + 1 : off[j + 1] - 1) {
      const uint32_t got = group_of(off.data(), (uint32_t)m, x);
      CHECK(got == j && off[got] <= x && x < off[got + 1], "%s: item %llu of group %zu found in %u", what, (unsigned long long)x, j, got);
      searched++;
    }
  // every bad array is refused
  if (m) {
    std::vector<uint64_t> bad = off;
    bad[0] = 1;
    CHECK(!encap_multi_offsets_ok(bad.data(), m, n), "%s: offsets[0] = 1 accepted", what);
    for (size_t j = 1; j <= m; j++) {
      if (off[j] == 0) continue;
      bad = off;
      bad[j - 1] = off[j] + 1;                    // decreasing at j (or, for j = 1, a first word that is not 0)
      CHECK(!encap_multi_offsets_ok(bad.data(), m, n), "%s: decreasing offset at %zu accepted", what, j);
      if (j > 8 && j + 8 < m) j += m / 16;
    }
    bad = off;
    bad[m] = off[m] + 1;
    CHECK(!encap_multi_offsets_ok(bad.data(), m, n), "%s: offsets[m] != n accepted", what);
  }
}

int main() {
  CHECK(!encap_multi_offsets_ok(nullptr, 0, 0), "null offsets accepted");
  {
    const uint64_t zero[2] = {0, 0};
    CHECK(encap_multi_offsets_ok(zero, 0, 0) && encap_multi_offsets_ok(zero, 1, 0), "the empty call refused");
    CHECK(encap_multi_plan(zero, 0, 8192).empty(), "m = 0 has pieces");
    const uint64_t big[2] = {0, (uint64_t)1 << 31};
    CHECK(!encap_multi_offsets_ok(big, 1, (size_t)1 << 31), "n = 2^31 accepted");
    CHECK(!encap_multi_offsets_ok(big, (size_t)1 << 31, 0), "m = 2^31 accepted");       // refused before a word is read
    const uint64_t top[2] = {0, ((uint64_t)1 << 31) - 1};
    CHECK(encap_multi_offsets_ok(top, 1, ((size_t)1 << 31) - 1), "n = 2^31 - 1 refused");
  }
  check_sizes({}, "no group");
  check_sizes({0}, "one empty group");
  check_sizes({1}, "m = 1");
  check_sizes({5}, "m = 1");
  check_sizes(std::vector<uint64_t>(300, 0), "all groups empty");
  check_sizes({0, 1, 0, 0, 62, 1, 64, 65, 0}, "group edges");
  check_sizes({100, 0, 156, 47}, "long tables");
  check_sizes({63, 64, 65, 1, 200}, "routes");
  check_sizes({8191, 8192, 8193}, "default threshold");
  check_sizes({(uint64_t)3 << 20}, "one huge group", false);
  check_sizes({0, 0, (uint64_t)1 << 21, 0, 3, 0}, "one huge group among small ones", false);
  {
    std::vector<uint64_t> alt;
    for (int j = 0; j < 257; j++) alt.push_back(j & 1);
    check_sizes(alt, "alternating empty groups and single items");
    for (auto& k : alt) k ^= 1;
    check_sizes(alt, "alternating single items and empty groups");
  }
  {
    std::vector<uint64_t> thousand(66, 1000);
    thousand.back() = 613;
    check_sizes(thousand, "groups of 1,000");
  }
  for (int round = 0; round < 400; round++) {
    const size_t m = 1 + next_u64() % (round < 200 ? 12 : 200);
    const uint64_t kind = next_u64() % 4;
    std::vector<uint64_t> sizes(m);
    for (auto& k : sizes) {
      const uint64_t v = next_u64();
      k = kind == 0 ? v % 4 : kind == 1 ? ((v & 3) ? 0 : (v >> 8) % 70) : kind == 2 ? (v >> 8) % 130 : ((v & 15) ? (v >> 8) % 5 : (v >> 8) % 9000);
    }
    check_sizes(sizes, "random");
  }
  printf("%zu offset arrays, %zu searches\n", arrays, searched);
  if (failures) { printf("%d checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
