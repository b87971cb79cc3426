// KZG verify_each (keaki_hip_kzg_verify_each), G1 side and the counting: one verdict per opening. By bilinearity the predicate of reference
// src/kzg.rs:135-148 for item i is
//     L_i = C_i - y_i g1 + z_i proof_i          valid_i  <=>  e(L_i, g2) * e(-proof_i, [tau]_2) == 1
// (z_i proof_i moved across the pairing, as verify_batch does). What lives here:
//   k_ve_g1        L_i and -proof_i in affine, one lane per item: y_i g1 from the context's window table of g1 (ec_batch.hip.h: fb_accumulate),
//                  z_i proof_i on the GLV ladder in 29-bit limbs (jac29.hip.h), two general additions -- either operand may be the identity, and
//                  C - y g1 = z proof (the doubling branch) and C - y g1 = -z proof (L the identity) are legal inputs -- and ONE inversion
//   k_ve_tau_inf   [tau]_2 = identity: e(-proof, [tau]_2) = 1 whatever the proof, so valid_i <=> L_i is the identity; no pairing runs
//   k_ve_count     the status bytes -> (count of ones, index of the first), added into the two words the codec's counters use
// The pairing itself is kzg_each_pair.hip.
#include "ec_batch.hip.h"
#include "kzg_fr.hip.h"
#include "internal.h"
namespace keaki_internal {
using namespace bn254;

// POINT_MODE 0: z_i = points[i]. POINT_MODE 1: z_i = omega^(first + i) with omega = points[0], raised per lane (at most 31 squarings and as many
// products in Fr beside a 254-bit ladder in G1): the n points never exist in memory.
template <int POINT_MODE>
static __global__ void __launch_bounds__(64) k_ve_g1(const G1Aff* __restrict__ coms, u32 com_stride, const G1Aff* __restrict__ tab_g1, FbShape g,
                                                     const Fr* __restrict__ points, const Fr* __restrict__ values, const G1Aff* __restrict__ proofs,
                                                     u32 first, u32 n, G1Aff* __restrict__ lhs_out, G1Aff* __restrict__ neg_proof_out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Aff proof = proofs[i];
  const Fr z = POINT_MODE ? fr_pow_u32(points[0], first + i) : points[i];
  u32 v[8];
  fp_from_mont<FrParams>(v, fp_neg<FrParams>(values[i]));
  const G1Xyzz yg = fb_accumulate(xyzz_inf<Fq>(), tab_g1, g, v);                              // (-y) g1
  const G1Jac a = jac_add(jac_from_aff(coms[(size_t)i * com_stride]), xyzz_to_jac(yg));      // C - y g1
  const G1Jac b = jac_scalar_mul_u29(jac_from_aff(proof), z);                                // z proof (the identity for proof = (0, 0) or z = 0)
  lhs_out[i] = jac_to_aff(jac_add(a, b));                                                    // the identity goes out as (0, 0)
  neg_proof_out[i] = aff_cneg(proof, !aff_is_inf(proof));
}

static __global__ void __launch_bounds__(256) k_ve_tau_inf(const G1Aff* __restrict__ lhs, u32 n, uint8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) status[i] = aff_is_inf(lhs[i]) ? 0 : 1;
}

// grid-stride over the bytes; a wave adds its lanes' counts and takes the minimum of their first indices by cross-lane moves, and only a wave
// that saw a one touches the counters
static __global__ void __launch_bounds__(256) k_ve_count(const uint8_t* __restrict__ status, u32 n, unsigned long long* __restrict__ bad2) {
  u32 count = 0, first = 0xFFFFFFFFu;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (status[i]) { count++; first = first < i ? first : i; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    count += (u32)__shfl_xor((int)count, off, 64);
    const u32 o = (u32)__shfl_xor((int)first, off, 64);
    first = first < o ? first : o;
  }
  if ((threadIdx.x & 63u) == 0 && count) {
    atomicAdd(bad2, (unsigned long long)count);
    atomicMin(bad2 + 1, (unsigned long long)first);
  }
}

keaki_status verify_each_g1_run(keaki_hip_ctx* ctx, const void* d_coms, int com_stride, const void* d_tab_g1, uint32_t wb, const void* d_points, int point_mode,
                                const void* d_values, const void* d_proofs, size_t first, size_t n, void* d_lhs_out, void* d_neg_proof_out) {
  if (n == 0) return KEAKI_OK;
  if (first + n >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_verify_each: n must be < 2^31 per call");
  const G1Aff* coms = (const G1Aff*)d_coms + (com_stride ? first : 0);
  const Fr* points = (const Fr*)d_points + (point_mode ? 0 : first);
  const Fr* values = (const Fr*)d_values + first;
  const G1Aff* proofs = (const G1Aff*)d_proofs + first;
  if (point_mode)
    hipLaunchKernelGGL(k_ve_g1<1>, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, coms, (u32)com_stride, (const G1Aff*)d_tab_g1, fb_shape(wb), points, values,
                       proofs, (u32)first, (u32)n, (G1Aff*)d_lhs_out, (G1Aff*)d_neg_proof_out);
  else
    hipLaunchKernelGGL(k_ve_g1<0>, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, coms, (u32)com_stride, (const G1Aff*)d_tab_g1, fb_shape(wb), points, values,
                       proofs, (u32)first, (u32)n, (G1Aff*)d_lhs_out, (G1Aff*)d_neg_proof_out);
  return launch_check(ctx, "verify_each_g1");
}

keaki_status verify_each_tau_inf_run(keaki_hip_ctx* ctx, const void* d_lhs, size_t n, void* d_status) {
  if (n == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_ve_tau_inf, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const G1Aff*)d_lhs, (u32)n, (uint8_t*)d_status);
  return launch_check(ctx, "verify_each_tau_inf");
}

keaki_status verify_each_count_run(keaki_hip_ctx* ctx, const void* d_status, size_t n, void* d_bad2) {
  if (n == 0) return KEAKI_OK;
  const u32 want = cdiv(n, 256 * 16), cap = ctx->n_cu * 4u;
  hipLaunchKernelGGL(k_ve_count, dim3(want < cap ? want : cap), dim3(256), 0, ctx->stream, (const uint8_t*)d_status, (u32)n, (unsigned long long*)d_bad2);
  return launch_check(ctx, "verify_each_count");
}

}  // namespace keaki_internal
