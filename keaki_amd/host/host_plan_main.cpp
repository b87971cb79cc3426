// The chunk plans of the host-array MSM and kzg_open (keaki_amd/csrc/host_plan.h: msm_pipe_bounds, open_plan) on a CPU, under
// AddressSanitizer / UBSan (make host_plan_asan; tests/test_host_plan_cpu.py): the invariants the device code relies on, over forced
// chunk counts, growth factors and lengths around every threshold, and the automatic bounds of the four benchmark lengths. Then the shrinking
// reservation of the KZG verdict calls (reserve_shrinking) under each of its four shrink rules, against a reservation that refuses above a byte limit.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../csrc/host_plan.h"

using namespace keaki_internal;

// the four chunking options with the defaults of struct Tuning (keaki_amd/csrc/internal.h, which needs HIP); the program prints them and
// tests/test_host_plan_cpu.py holds them against that struct
struct Tuning {
  int msm_pipe_chunks = -1;
  bool pipe_chunks = true;
  long long msm_pipe_min = 1 << 20;
  int msm_pipe_growth = 160;
};

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                            \
  } while (0)

// the four sites of reserve_shrinking (keaki_amd/csrc/api_kzg.hip) with their floors and shrink rules, restated: verify_each_core | coset_pairs_core
// (coset_rows_plan.h: cr_chunk_halve) | set_pairs_core (set_rows_plan.h: sr_chunk_halve) | set_each_reserve (set_rows_plan.h: SE_CHUNK_MIN, se_chunk_halve)
static size_t shrink_each(size_t ch) { return std::max<size_t>(32, ((ch + 1) / 2 + 31) & ~(size_t)31); }
static size_t shrink_half(size_t ch) { return (ch + 1) / 2; }
static size_t shrink_set_each(size_t ch) { const size_t h = ((ch + 1) / 2 + 31) & ~(size_t)31; return h < 32 ? 32 : h; }
static const struct ShrinkSite { const char* name; size_t floor; size_t (*shrink)(size_t); } SITES[] = {
    {"verify_each_core", 32, shrink_each}, {"coset_pairs_core", 1, shrink_half}, {"set_pairs_core", 1, shrink_half}, {"set_each_reserve", 32, shrink_set_each}};
enum Status { OK = 0, REFUSED = 3, OTHER = 5 };

// one run: a reservation of `per_item` bytes per item that refuses above `limit` bytes (or fails with OTHER at the first try); what was tried, in order
struct ShrinkRun { std::vector<size_t> tried; size_t cleared = 0, ch = 0; Status st = OK; };
static ShrinkRun shrink_run(const ShrinkSite& s, size_t start, size_t per_item, size_t limit, bool other) {
  ShrinkRun r;
  r.ch = start;
  r.st = reserve_shrinking(REFUSED, r.ch, s.floor, s.shrink,
                           [&](size_t c) { r.tried.push_back(c); return other || r.tried.size() > 64 ? OTHER : c * per_item > limit ? REFUSED : OK; },      // 64 tries: a loop that does not end
                           [&] { r.cleared++; });
  return r;
}
static size_t check_shrinking() {
  size_t runs = 0;
  const size_t per_item = 192;
  for (const ShrinkSite& s : SITES)
    for (size_t start : {(size_t)1, s.floor, s.floor + 1, (size_t)33, (size_t)64, (size_t)65, (size_t)70, (size_t)4096}) {
      // the counts the rule visits from `start`: strictly decreasing, and below `start` never below the floor
      std::vector<size_t> seq{start};
      while (seq.back() > s.floor) {
        const size_t next = s.shrink(seq.back());
        CHECK(next < seq.back() && next >= s.floor, "%s: start %zu, %zu -> %zu", s.name, start, seq.back(), next);
        if (next >= seq.back()) return runs;       // the loop below would not end
        seq.push_back(next);
      }
      // a limit for every count from the floor (or a start below it) up to the start: the first count of the sequence that fits is accepted, and it is the last try
      for (size_t fits = std::min(s.floor, start); fits <= start; fits++, runs++) {
        const ShrinkRun r = shrink_run(s, start, per_item, fits * per_item, false);
        const size_t want = std::find_if(seq.begin(), seq.end(), [&](size_t c) { return c <= fits; }) - seq.begin();
        CHECK(want < seq.size() && r.st == OK && r.ch == seq[want], "%s: start %zu, %zu fit: status %d, accepted %zu", s.name, start, fits, (int)r.st, r.ch);
        CHECK(r.tried == std::vector<size_t>(seq.begin(), seq.begin() + want + 1) && r.cleared == want, "%s: start %zu, %zu fit: %zu tries, %zu clears", s.name, start,
              fits, r.tried.size(), r.cleared);
      }
      // nothing fits: every count of the sequence is tried once, and the refusal at the floor is what the caller gets
      const ShrinkRun none = shrink_run(s, start, per_item, per_item - 1, false);
      CHECK(none.st == REFUSED && none.tried == seq && none.cleared + 1 == seq.size() && none.ch == seq.back(), "%s: start %zu, nothing fits: status %d after %zu tries",
            s.name, start, (int)none.st, none.tried.size());
      // another failure comes back after one try, with the recorded error left alone
      const ShrinkRun other = shrink_run(s, start, per_item, 0, true);
      CHECK(other.st == OTHER && other.tried == std::vector<size_t>{start} && other.cleared == 0, "%s: start %zu, other failure: status %d after %zu tries, %zu clears",
            s.name, start, (int)other.st, other.tried.size(), other.cleared);
      runs += 2;
    }
  return runs;
}

int main() {
  std::vector<size_t> ns;
  for (size_t n = 0; n < 400; n++) ns.push_back(n);
  for (size_t n : {(size_t)65535, (size_t)65536, (size_t)65537, (size_t)1 << 20, ((size_t)1 << 20) + 1, ((size_t)1 << 21) - 1, (size_t)1 << 22, ((size_t)1 << 24) + 5})
    ns.push_back(n);
  size_t plans = 0;
  for (int growth : {50, 100, 160, 400, 1000})
    for (int chunks : {2, 3, 4, 7, 16, 64, 65, 1000})
      for (size_t n : ns) {
        Tuning t;
        t.msm_pipe_growth = growth;
        t.msm_pipe_chunks = chunks;
        const std::vector<size_t> b = msm_pipe_bounds(t, n);
        CHECK(b.size() >= 2 && b.front() == 0 && b.back() == n, "growth %d chunks %d n %zu", growth, chunks, n);
        CHECK(b.size() - 1 <= 64, "growth %d chunks %d n %zu: %zu pieces", growth, chunks, n, b.size() - 1);
        for (size_t j = 0; j + 1 < b.size(); j++) {
          if (n >= 1) CHECK(b[j] < b[j + 1], "growth %d chunks %d n %zu: bound %zu", growth, chunks, n, j);
          if (n >= 65536 && j >= 1) CHECK(b[j] % 4096 == 0, "growth %d chunks %d n %zu: bound %zu = %zu", growth, chunks, n, j, b[j]);
        }
        const OpenPlan p = open_plan(t, n);
        CHECK(p.chunks.size() == p.ranges.size() && p.chunks.size() != 1, "growth %d chunks %d n %zu", growth, chunks, n);
        if (p.chunks.size() >= 2 && n >= 2) {
          plans++;
          // the coefficient chunks partition [0, n), top first
          CHECK(p.chunks.front().second == n && p.chunks.back().first == 0, "growth %d chunks %d n %zu", growth, chunks, n);
          for (size_t j = 0; j < p.chunks.size(); j++) {
            CHECK(p.chunks[j].first < p.chunks[j].second, "growth %d chunks %d n %zu: chunk %zu", growth, chunks, n, j);
            if (j) CHECK(p.chunks[j].second == p.chunks[j - 1].first, "growth %d chunks %d n %zu: chunk %zu", growth, chunks, n, j);
          }
          // the MSM ranges are non-empty and partition [0, n - 1), top first as well
          size_t top = n - 1;
          for (size_t j = 0; j < p.ranges.size(); j++) {
            CHECK(p.ranges[j].second >= 1, "growth %d chunks %d n %zu: range %zu is empty", growth, chunks, n, j);
            CHECK(p.ranges[j].first + p.ranges[j].second == top, "growth %d chunks %d n %zu: range %zu", growth, chunks, n, j);
            top = p.ranges[j].first;
          }
          CHECK(top == 0, "growth %d chunks %d n %zu: the ranges end at %zu", growth, chunks, n, top);
        }
      }
  CHECK(plans > 10000, "only %zu chunked open plans were checked", plans);
  // the automatic bounds (default tuning) at the lengths the chunked paths were measured at
  const struct { size_t n; std::vector<size_t> bounds; } pinned[] = {
      {(size_t)1 << 20, {0, 200704, 524288, 1048576}},
      {(size_t)1 << 21, {0, 225280, 585728, 1167360, 2097152}},
      {(size_t)1 << 22, {0, 155648, 413696, 819200, 1474560, 2519040, 4194304}},
      {(size_t)1 << 24, {0, 634880, 1654784, 3289088, 5902336, 10084352, 16777216}},
  };
  for (const auto& c : pinned) CHECK(msm_pipe_bounds(Tuning(), c.n) == c.bounds, "automatic bounds at n = %zu", c.n);
  // open chunks automatically from 2^21 coefficients on, the MSM from 2^20 scalars on
  CHECK(!open_plan(Tuning(), ((size_t)1 << 21) - 1).chunked() && open_plan(Tuning(), (size_t)1 << 21).chunks.size() == 4, "open threshold");
  CHECK(msm_pipe_bounds(Tuning(), ((size_t)1 << 20) - 1).size() == 2, "msm threshold");
  const size_t shrink_runs = check_shrinking();
  CHECK(shrink_runs > 4 * 4096, "only %zu shrinking reservations were checked", shrink_runs);
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  const Tuning d;
  printf("defaults: msm_pipe_chunks=%d pipe_chunks=%d msm_pipe_min=%lld msm_pipe_growth=%d\n", d.msm_pipe_chunks, (int)d.pipe_chunks, d.msm_pipe_min, d.msm_pipe_growth);
  printf("all checks passed (%zu chunked open plans)\n", plans);
  return 0;
}
