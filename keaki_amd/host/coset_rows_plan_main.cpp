// Prints the host plan of kzg coset_pairs (csrc/coset_rows_plan.h) for tests/test_coset_rows_plan_cpu.py, which holds every line against the plan
// restated in tests/coset_pairs_model.py. Includes that header and nothing of HIP.
#include <cstdio>
#include <initializer_list>

#include "../csrc/coset_rows_plan.h"

using namespace keaki_internal;

int main() {
  for (uint32_t log2l = 0; log2l <= 10; log2l++) {
    const uint32_t wb = cr_wb(log2l);
    std::printf("table %u %u %u %u %zu\n", log2l, wb, cr_windows(wb), cr_entries(wb), cr_table_bytes(log2l, wb));
    for (uint32_t c : CR_WB_CANDIDATES) std::printf("bytes %u %u %zu\n", log2l, c, cr_table_bytes(log2l, c));
    const uint64_t ns[] = {1, 2, 63, 64, 2047, 2048, 2049, 4096, 131071, 131072, 131073, 1u << 20};
    const uint64_t opts[] = {0, 1, 4, 4096, (uint64_t)1 << 31};
    for (uint64_t n : ns)
      for (uint64_t o : opts) std::printf("slices %u %llu %llu %u\n", log2l, (unsigned long long)n, (unsigned long long)o, cr_slices(n, log2l, o));
    const size_t ms[] = {1, 1023, 1024, 1025, ((size_t)1 << 20) - 1, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)1 << 30};
    for (size_t m : ms) std::printf("chunk %u %zu %zu\n", log2l, m, cr_chunk_items(m, log2l));
    for (int r = 0; r <= 2; r++) std::printf("route %u %d %d\n", log2l, r, cr_route(r, log2l));
  }
  for (size_t ch : {(size_t)1, (size_t)2, (size_t)3, (size_t)1024, (size_t)1025}) std::printf("halve %zu %zu\n", ch, cr_chunk_halve(ch));
  std::printf("consts %zu %u %zu\n", CR_TABLE_BYTES_MAX, CR_MIN_LANES, CR_CHUNK_VALUES);
  return 0;
}
