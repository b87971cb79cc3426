// Prints the host plan of kzg set_pairs (csrc/set_rows_plan.h) for tests/test_set_rows_plan_cpu.py, which holds every line against the plan
// restated in tests/set_pairs_model.py. Includes that header and nothing of HIP.
#include <cstdio>
#include <initializer_list>

#include "../csrc/set_rows_plan.h"

using namespace keaki_internal;

int main() {
  for (size_t k = 1; k <= 64; k++) {
    const uint32_t wb = sr_wb(k), log2kp = sr_log2kp(k);
    std::printf("table %zu %u %u %u %zu %u\n", k, wb, sr_windows(wb), sr_entries(wb), sr_table_bytes(k, wb), log2kp);
    for (uint32_t c : SR_WB_CANDIDATES) std::printf("bytes %zu %u %zu\n", k, c, sr_table_bytes(k, c));
    for (int pm = 0; pm <= 1; pm++)
      for (int msm = 0; msm <= 1; msm++) std::printf("item %zu %d %d %zu\n", k, pm, msm, sr_item_bytes(k, log2kp, pm, msm != 0));
  }
  for (uint32_t log2kp = 0; log2kp <= 6; log2kp++) {
    const uint64_t ns[] = {1, 2, 63, 64, 2047, 2048, 2049, 4096, 131071, 131072, 131073, 1u << 20};
    const uint64_t opts[] = {0, 1, 4, 4096, (uint64_t)1 << 31};
    for (uint64_t n : ns)
      for (uint64_t o : opts) std::printf("slices %u %llu %llu %u\n", log2kp, (unsigned long long)n, (unsigned long long)o, sr_slices(n, log2kp, o));
    const size_t ms[] = {1, 1023, 1024, 1025, ((size_t)1 << 20) - 1, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)1 << 30};
    for (size_t m : ms) std::printf("chunk %u %zu %zu\n", log2kp, m, sr_chunk_items(m, log2kp));
  }
  for (uint32_t wb : {13u, 10u, 8u}) std::printf("narrower %u %u\n", wb, sr_wb_narrower(wb));
  for (size_t ch : {(size_t)1, (size_t)2, (size_t)3, (size_t)1024, (size_t)1025}) std::printf("halve %zu %zu\n", ch, sr_chunk_halve(ch));
  for (size_t n : {(size_t)1, (size_t)31, (size_t)32, (size_t)65535, (size_t)65536, (size_t)65537, (size_t)1 << 20})
    std::printf("each %zu %zu %zu\n", n, se_chunk_items(n, (size_t)1 << 17), se_chunk_halve(se_chunk_items(n, (size_t)1 << 17)));
  for (int r = 0; r <= 2; r++)
    for (size_t n : {(size_t)1, (size_t)1 << 20}) std::printf("route %d %zu %d\n", r, n, se_route(r, n));
  std::printf("eachbytes %zu %zu\n", se_item_bytes(false), se_item_bytes(true));
  std::printf("consts %zu %u %zu %zu\n", SR_TABLE_BYTES_MAX, SR_MIN_LANES, SR_CHUNK_VALUES, SE_CHUNK_MIN);
  return 0;
}
