// The chunk plans of the host-array MSM and kzg_open (keaki_amd/csrc/host_plan.h: msm_pipe_bounds, open_plan) on a CPU, under
// AddressSanitizer / UBSan (make host_plan_asan; tests/test_host_plan_cpu.py): the invariants the device code relies on, over forced
// chunk counts, growth factors and lengths around every threshold, and the automatic bounds of the four benchmark lengths.
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
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  const Tuning d;
  printf("defaults: msm_pipe_chunks=%d pipe_chunks=%d msm_pipe_min=%lld msm_pipe_growth=%d\n", d.msm_pipe_chunks, (int)d.pipe_chunks, d.msm_pipe_min, d.msm_pipe_growth);
  printf("all checks passed (%zu chunked open plans)\n", plans);
  return 0;
}
