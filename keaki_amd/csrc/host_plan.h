// How the host-array MSM and kzg_open cut their input into chunks, and how a refused reservation shrinks: integer work alone. No HIP call and no
// HIP header, so keaki_amd/host/host_plan_main.cpp checks the invariants on a CPU (tests/test_host_plan_cpu.py). `T` is Tuning
// (internal.h) in the library; the functions read its members msm_pipe_chunks, pipe_chunks, msm_pipe_min and msm_pipe_growth only, and
// the plan program passes a struct of those four.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace keaki_internal {

// Chunk bounds of a host-pointer MSM over n scalars: b[0] = 0 < b[1] < ... < b.back() = n, one piece (two bounds) when the call is not
// chunked. Chunks GROW (the copy is faster than the kernels, so a short first chunk starts the device early and every later copy still
// finishes before the device asks for it).
template <class T>
std::vector<size_t> msm_pipe_bounds(const T& t, size_t n) {
  size_t k = 1;
  if (t.msm_pipe_chunks >= 2) k = (size_t)t.msm_pipe_chunks;
  else if (t.msm_pipe_chunks < 0 && t.pipe_chunks && n >= (size_t)t.msm_pipe_min) k = n >= ((size_t)1 << 22) ? 6 : n >= ((size_t)1 << 21) ? 4 : 3;      // measured: profiles/r05_msm_pipe_sweep_*.txt
  if (k > 64) k = 64;
  if (k > n) k = n ? n : 1;
  std::vector<size_t> b{0};
  if (k >= 2) {
    const double g = std::max(100, std::min(400, t.msm_pipe_growth)) / 100.0;
    double tot = 0, w = 1;
    for (size_t j = 0; j < k; j++, w *= g) tot += w;
    double acc = 0;
    w = 1;
    for (size_t j = 0; j + 1 < k; j++, w *= g) {
      acc += w;
      size_t e = (size_t)((double)n * acc / tot);
      if (n >= 65536) e &= ~(size_t)4095;                   // whole pages of scalars, whole tiles of the first sort
      if (e > b.back() && e < n) b.push_back(e);
    }
  }
  b.push_back(n);
  return b;
}

// Chunked kzg_open over n coefficients. Long polynomials come up in chunks FROM THE TOP (the quotient's recurrence Q_i = c_i + z Q_(i+1)
// runs downwards): `chunks` are the coefficient ranges [lo, hi), top first, `ranges` what each one gives the MSM (MsmPipe::ranges:
// q_i = Q_(i+1), so chunk [lo, hi) yields q_(lo-1) .. q_(hi-2)). Both are empty when the call runs with one copy in front.
// (automatic from 2^21 coefficients on: the first chunk's quotient stays in front of the first pass; 2^20: 2.71 ms in three chunks against 2.64
// with the copy in front, 2^21: 4.05 / 4.36, 2^22: 6.43 / 8.10, 2^24: 19.2 / 28.0 ms -- profiles/r05_open_chunked.txt)
struct OpenPlan {
  std::vector<std::pair<size_t, size_t>> chunks, ranges;
  bool chunked() const { return !chunks.empty(); }
};
template <class T>
OpenPlan open_plan(const T& t, size_t n) {
  OpenPlan p;
  if (!(t.msm_pipe_chunks >= 2 || (t.msm_pipe_chunks < 0 && t.pipe_chunks && n >= ((size_t)1 << 21)))) return p;     // "pipe_chunks" = 0 or "msm_pipe_chunks" = 0 / 1: one copy in front, on the context's stream
  const std::vector<size_t> bounds = msm_pipe_bounds(t, n);
  if (bounds.size() <= 2) return p;
  for (size_t j = 0; j + 1 < bounds.size(); j++) p.chunks.push_back({n - bounds[j + 1], n - bounds[j]});
  if (p.chunks.back().second == 1) { p.chunks[p.chunks.size() - 2].first = 0; p.chunks.pop_back(); }     // the lowest chunk must leave a quotient coefficient
  if (p.chunks.size() <= 1) { p.chunks.clear(); return p; }
  for (const auto& c : p.chunks) p.ranges.push_back({c.first ? c.first - 1 : 0, c.second - 1 - (c.first ? c.first - 1 : 0)});
  return p;
}

// A reservation for `ch` items that shrinks until it fits (the launch chunks of the KZG verdict calls, api_kzg.hip): try_reserve(ch) is called
// until it gives something other than `refused`, which is returned at once -- success with `ch` the count that fits; `refused` itself is
// returned when ch is at the floor. In between the recorded error is cleared and ch = shrink(ch), the site's own rule (strictly smaller, not below the floor).
// The status type is what try_reserve returns; `refused` is compared with it.
template <class Refused, class Shrink, class TryReserve, class ClearError>
auto reserve_shrinking(Refused refused, size_t& ch, size_t floor, Shrink shrink, TryReserve try_reserve, ClearError clear_error) {
  for (;;) {
    const auto st = try_reserve(ch);
    if (st != refused || ch <= floor) return st;
    clear_error();
    ch = shrink(ch);
  }
}

}  // namespace keaki_internal
