// encap_multi / encrypt_multi, G1 side: encapsulate to MANY commitments in one launch (reference src/kem.rs:22,30 inside the loop of
// src/vec.rs:63-66, once per receiver). Item i of group j needs P_i = r_i (C_j - beta_i g1) = r_i C_j + (-(r_i beta_i)) g1: the first term is a
// scalar multiple of a base that changes from group to group (the GLV ladder in 29-bit limbs, jac29.hip.h), the second a fixed-base sum over
// the context's window table of g1 (ec_batch.hip.h: fb_accumulate). One general addition joins them -- either term may be the identity, and
// they are equal for C = -beta g1, opposite for C = beta g1 -- and ONE conversion to affine ends the lane: one field inversion per item.
// (k_encap_g1 of the single-commitment path walks two ladders and inverts twice.) No table per commitment is built anywhere.
#include "ec_batch.hip.h"
#include "internal.h"
namespace keaki_internal {
using namespace bn254;

// offsets: m + 1 words, non-decreasing, offsets[0] <= first and first + n <= offsets[m] (api.hip validates the caller's array before any
// launch). The search keeps offsets[lo] <= gi < offsets[hi] and reads words 1 .. m - 1 only, so the group it returns is below m whatever
// the array holds; with empty groups around it, it ends on the one non-empty group that holds the item.
static __global__ void __launch_bounds__(64) k_encap_multi_g1(const G1Aff* __restrict__ coms, const unsigned long long* __restrict__ offsets, u32 m,
                                                              unsigned long long first, const G1Aff* __restrict__ tab_g1, FbShape g,
                                                              const Fr* __restrict__ values, const Fr* __restrict__ rs, u32 n, G1Aff* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long gi = first + i;
  u32 lo = 0, hi = m;
  while (hi - lo > 1u) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= gi) lo = mid; else hi = mid;
  }
  const G1Aff com = coms[lo];
  const Fr r = rs[i];
  const G1Jac a = jac_scalar_mul_u29(jac_from_aff(com), r);                       // r C_j (the identity for C_j = (0, 0) or r = 0)
  u32 v[8];
  fp_from_mont<FrParams>(v, fp_neg<FrParams>(fp_mul<FrParams>(r, values[i])));
  const G1Xyzz b = fb_accumulate(xyzz_inf<Fq>(), tab_g1, g, v);                     // (-(r beta)) g1
  out[i] = jac_to_aff(jac_add(a, xyzz_to_jac(b)));                                // the identity goes out as (0, 0): GT one in the pairing
}

keaki_status encap_multi_g1_run(keaki_hip_ctx* ctx, const void* d_coms, const void* d_offsets, size_t m, uint64_t first, const void* d_tab_g1, uint32_t wb,
                                const void* d_values, const void* d_r, size_t n, void* d_out) {
  if (n == 0) return KEAKI_OK;
  if (m == 0 || m >= ((size_t)1 << 31) || n >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_multi_g1: %zu items in %zu groups", n, m);
  hipLaunchKernelGGL(k_encap_multi_g1, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, (const G1Aff*)d_coms, (const unsigned long long*)d_offsets, (u32)m,
                     (unsigned long long)first, (const G1Aff*)d_tab_g1, fb_shape(wb), (const Fr*)d_values, (const Fr*)d_r, (u32)n, (G1Aff*)d_out);
  return launch_check(ctx, "encap_multi_g1");
}
}  // namespace keaki_internal
