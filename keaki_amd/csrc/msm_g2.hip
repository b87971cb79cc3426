// G2 instantiation of the MSM pipeline (no call site in keaki; requested by the north star).
#define KEAKI_FQ2_OUTLINE 1
#include "msm_host.hip.h"
namespace keaki_internal {
// internal.h's widest forced windows against the plans (a check only; kept out of the MSM kernel sources, whose hash stamps the profiles):
// a target is accepted exactly when its plan leaves at most PART_MAX_BINS x 2^PART_MAX_FINE_SHIFT buckets to sort -- all windows' without
// tables, the largest window's with them
constexpr size_t msm_sort_buckets(int c_target, bool shared) {
  const u32 W = (254 + c_target - 1) / c_target, base = 254 / W, rem = 254 % W, c = rem ? base + 1 : base, k = rem ? rem : W;
  size_t nb = 0, mb = 0;
  for (u32 w = 0; w < W; w++) {
    const u32 wd = w < k ? c : c - 1;
    const size_t b = (size_t)1 << (w == W - 1 ? wd : wd - 1);
    nb += b; mb = b > mb ? b : mb;
  }
  return shared ? mb : nb;
}
constexpr bool msm_c_limit_is(int max, bool shared) {
  for (int c = 3; c <= 24; c++)
    if ((msm_sort_buckets(c, shared) <= ((size_t)PART_MAX_BINS << PART_MAX_FINE_SHIFT)) != (c <= max)) return false;
  return true;
}
static_assert(msm_c_limit_is(MSM_C_MAX, false) && msm_c_limit_is(MSM_C_SHARED_MAX, true), "internal.h: MSM_C_MAX / MSM_C_SHARED_MAX");

keaki_status msm_g2_run(keaki_hip_ctx* ctx, const void* d_points, size_t srs_len, const void* d_scalars, size_t n, void* d_out_jac, const void* d_table,
                        int c_table, const MsmPipe* pipe) {
  return msm_dev<Fq2>(ctx, (const G2Aff*)d_points, srs_len, d_scalars, n, d_out_jac, (const G2Aff*)d_table, c_table, pipe);
}
// window tables of a fixed G2 basis: all windows share one bucket set, and the per-window Horner doublings -- a serial chain of ~240
// Fq2 doublings on one lane, 4.4 ms -- disappear (profiles/r02_msm_g2_kernel_stats.csv)
keaki_status msm_g2_precompute_run(keaki_hip_ctx* ctx, const void* d_points, size_t N, int* c_table_out, size_t* table_bytes_out, void** d_table_out) {
  return msm_precompute<Fq2>(ctx, d_points, N, c_table_out, table_bytes_out, d_table_out);
}
}  // namespace keaki_internal
