// KZG batch verification (keaki_hip_kzg_verify_batch): the scalar-field side and the final combination of the random linear combination
//     L = sum gamma_i C_i - (sum gamma_i y_i) g1 + sum (gamma_i z_i) proof_i        R = sum gamma_i proof_i
// which is sum gamma_i x (the predicate of reference src/kzg.rs:135-148, with z_i proof_i moved across the pairing). The group sums are the
// library's MSM over the proofs as an ad-hoc base vector (api.hip enqueues them); what lives here:
//   k_vb_prepare   s_i = gamma_i z_i (the second MSM's scalars) and the per-workgroup partial sums of t = sum gamma_i y_i, g = sum gamma_i
//   k_vb_finish    the partials of all workgroups -> (g, -t), one workgroup
//   k_vb_aff_to_jac / k_vb_jac_to_aff   layout moves around the final sum L = K + M + (-t) g1 (g1_sum_run) and into the pairing's slots
// Fr addition is exact, so the order of the reduction does not matter: every sum is the canonical Montgomery residue.
#include <algorithm>
#include "internal.h"
#include "bn254_curve.hip.h"
#include "kzg_fr.hip.h"

namespace bn254 {

constexpr u32 VB_THREADS = 256, VB_WAVES = VB_THREADS / 64;

// (g, t) of the workgroup -> out2[0], out2[1]: one partial per wave through LDS, thread 0 adds the VB_WAVES of them
KDEV void fr_block_sum2(Fr g, Fr t, Fr* __restrict__ out2) {
  __shared__ Fr sh[2 * VB_WAVES];
  g = fr_wave_sum(g);
  t = fr_wave_sum(t);
  const u32 wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { sh[2 * wave] = g; sh[2 * wave + 1] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Fr sg = sh[0], st = sh[1];
#pragma unroll
    for (u32 w = 1; w < VB_WAVES; w++) { sg = fp_add<FrParams>(sg, sh[2 * w]); st = fp_add<FrParams>(st, sh[2 * w + 1]); }
    out2[0] = sg;
    out2[1] = st;
  }
}

// Grid-stride over the n items. POINT_MODE 0: z_i = points[i]. POINT_MODE 1: z_i = omega^i with omega = points[0] -- the lane raises omega to its
// first index once and then steps by omega^(lanes of the grid); the n points never exist in memory.
// 96 B in (64 B in mode 1), 32 B out per item and three Fr products: bound by memory, not by the multiplier.
template <int POINT_MODE>
static __global__ void __launch_bounds__(VB_THREADS) k_vb_prepare(const Fr* __restrict__ gammas, const Fr* __restrict__ points, const Fr* __restrict__ values,
                                                                  u32 n, Fr* __restrict__ s_out, Fr* __restrict__ partials) {
  const u32 first = blockIdx.x * VB_THREADS + threadIdx.x, lanes = gridDim.x * VB_THREADS;
  Fr g = fp_zero<FrParams>(), t = fp_zero<FrParams>();
  Fr z = fp_zero<FrParams>(), step = z;
  if constexpr (POINT_MODE == 1) {
    if (first < n) {
      const Fr omega = points[0];
      z = fr_pow_u32(omega, first);
      step = fr_pow_u32(omega, lanes);
    }
  }
#pragma unroll 1
  for (u32 i = first; i < n; i += lanes) {
    const Fr gamma = gammas[i];
    if constexpr (POINT_MODE == 0) z = points[i];
    s_out[i] = fp_mul<FrParams>(gamma, z);
    t = fp_add<FrParams>(t, fp_mul<FrParams>(gamma, values[i]));
    g = fp_add<FrParams>(g, gamma);
    if constexpr (POINT_MODE == 1) z = fp_mul<FrParams>(z, step);
  }
  fr_block_sum2(g, t, partials + 2 * (size_t)blockIdx.x);
}

// out2 = (g, -t) from the sum of the `blocks` partial pairs, one workgroup (-t: the scalar of g1 in L)
static __global__ void __launch_bounds__(VB_THREADS) k_vb_finish(const Fr* __restrict__ partials, u32 blocks, Fr* __restrict__ out2) {
  Fr g = fp_zero<FrParams>(), t = fp_zero<FrParams>();
#pragma unroll 1
  for (u32 b = threadIdx.x; b < blocks; b += VB_THREADS) {
    g = fp_add<FrParams>(g, partials[2 * (size_t)b]);
    t = fp_add<FrParams>(t, partials[2 * (size_t)b + 1]);
  }
  fr_block_sum2(g, t, out2);
  if (threadIdx.x == 0) out2[1] = fp_neg<FrParams>(out2[1]);       // thread 0 wrote it
}

// The combination L = K + M - t g1 is the library's own sum of normalised Jacobian points (g1_sum_run); these two move the operands between
// the layouts: affine results of the scalar-mult kernel -> normalised Jacobian (x, y, 1) / (1, 1, 0), and the two sums back to the affine
// first-argument slots of the pairing. No arithmetic.
static __global__ void __launch_bounds__(64) k_vb_aff_to_jac(const G1Aff* __restrict__ in, u32 n, Fq* __restrict__ out_jac) {
  const u32 i = threadIdx.x;
  if (blockIdx.x != 0 || i >= n) return;
  const G1Aff p = in[i];
  const bool inf = aff_is_inf(p);
  out_jac[3 * i] = inf ? fq_one() : p.x;
  out_jac[3 * i + 1] = inf ? fq_one() : p.y;
  out_jac[3 * i + 2] = inf ? fq_zero() : fq_one();
}
static __global__ void __launch_bounds__(64) k_vb_jac_to_aff(const Fq* __restrict__ l_jac, const Fq* __restrict__ r_jac, G1Aff* __restrict__ out2) {
  const u32 i = threadIdx.x;
  if (blockIdx.x != 0 || i >= 2) return;
  const Fq* p = i ? r_jac : l_jac;
  const bool inf = f_is_zero(p[2]);
  G1Aff a;
  a.x = inf ? fq_zero() : p[0];
  a.y = inf ? fq_zero() : p[1];
  out2[i] = a;
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

size_t verify_batch_partials_bytes() { return (size_t)VB_MAX_BLOCKS * 2 * sizeof(Fr); }

keaki_status verify_batch_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const void* d_values, size_t n,
                                      void* d_s_out, void* d_partials, void* d_gt_out) {
  if (n == 0 || n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_verify_batch: n must be in 1 .. 2^31 - 1 on the device side");
  const u32 want = cdiv(n, VB_THREADS), cap = std::min<u32>(VB_MAX_BLOCKS, ctx->n_cu * 4u);
  const u32 blocks = want < cap ? want : cap;
  if (point_mode)
    hipLaunchKernelGGL(k_vb_prepare<1>, dim3(blocks), dim3(VB_THREADS), 0, ctx->stream, (const Fr*)d_gammas, (const Fr*)d_points, (const Fr*)d_values, (u32)n,
                       (Fr*)d_s_out, (Fr*)d_partials);
  else
    hipLaunchKernelGGL(k_vb_prepare<0>, dim3(blocks), dim3(VB_THREADS), 0, ctx->stream, (const Fr*)d_gammas, (const Fr*)d_points, (const Fr*)d_values, (u32)n,
                       (Fr*)d_s_out, (Fr*)d_partials);
  hipLaunchKernelGGL(k_vb_finish, dim3(1), dim3(VB_THREADS), 0, ctx->stream, (const Fr*)d_partials, blocks, (Fr*)d_gt_out);
  return launch_check(ctx, "verify_batch_scalars");
}

keaki_status verify_batch_aff_to_jac_run(keaki_hip_ctx* ctx, const void* d_in_aff, uint32_t n, void* d_out_jac) {
  if (n > 64) return fail(ctx, KEAKI_ERR_BAD_ARG, "verify_batch_aff_to_jac: at most 64 points");
  hipLaunchKernelGGL(k_vb_aff_to_jac, dim3(1), dim3(64), 0, ctx->stream, (const G1Aff*)d_in_aff, n, (Fq*)d_out_jac);
  return launch_check(ctx, "verify_batch_aff_to_jac");
}
keaki_status verify_batch_jac_to_aff_run(keaki_hip_ctx* ctx, const void* d_l_jac, const void* d_r_jac, void* d_out_lr_aff) {
  hipLaunchKernelGGL(k_vb_jac_to_aff, dim3(1), dim3(64), 0, ctx->stream, (const Fq*)d_l_jac, (const Fq*)d_r_jac, (G1Aff*)d_out_lr_aff);
  return launch_check(ctx, "verify_batch_jac_to_aff");
}

}  // namespace keaki_internal
