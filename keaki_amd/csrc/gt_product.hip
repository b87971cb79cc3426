// GT product (keaki_hip_pairing_product): the product of n Fq12 Miller-loop outputs, so that ONE final exponentiation serves n pairings:
//     prod_i e(P_i, Q_i) = FE(prod_i miller(P_i, Q_i)).
// Elements come and go in the representation keaki_hip_miller_loop_batch documents (12 Fq per element, 2^256 Montgomery form, slot 2k + parity = Fq2
// coefficient k, component parity); inside, two lanes hold an element in the 2^261 form and multiply with the shipped fq12_mul (pair261.hip.h), whose
// device functions run here as they are. A translation unit of its own: the pairing kernels' generated code does not depend on this kernel in any way.
//   k_gt_product  a workgroup of 64 lanes = 32 lane pairs. A pair multiplies up the elements base + pair of the workgroup's strips (grid-stride, the
//                 trip count uniform per workgroup: a pair past n multiplies by one, all 64 lanes stay active for the lane-pair exchanges), then the 32
//                 accumulators are folded by a tree in LDS (5 levels; every pair multiplies at every level, the pairs a level no longer needs compute
//                 values nobody reads) and pair 0 writes ONE element. n <= GP_ONE_BLOCK: one workgroup, one launch; more: up to GP_MAX_BLOCKS
//                 workgroups write partial products and a second launch of one workgroup folds those. Fq12 products are exact and commute: neither the
//                 split nor the order changes a bit of the result.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this file): k_gt_product 256 VGPRs + 12 AGPRs (one wave per SIMD: the kernel
// runs at most 256 workgroups of one wave, so occupancy buys nothing), 36,864 B LDS (12 KB parking area, two 12 KB buffers of the tree), no scratch
// memory, no atomics. k_gt_pair_product (the pairwise mode of kzg verify_sets_each: out[i] = a[i] b[i], no tree) 232 VGPRs, 12,288 B LDS, no scratch memory.
#define KEAKI_FQ2_OUTLINE 1
#include <algorithm>
#include "internal.h"
#include "pairing.hip.h"
namespace keaki_internal {
using namespace bn254;

constexpr u32 GP_PAIRS = 32;                  // lane pairs of a workgroup
constexpr u32 GP_ONE_BLOCK = 4 * GP_PAIRS;    // elements up to which one workgroup takes the whole product
constexpr u32 GP_MAX_BLOCKS = 256;            // partial products of the first launch

// The second operand of a product stays in memory (fq12_mul_ld: its halves are loaded when a partial product needs them, the first two partial
// products wait in LDS): with both operands in registers the kernel kept 160 bytes per lane in scratch memory.
static __global__ void __launch_bounds__(64) k_gt_product(const Fq* __restrict__ in, u32 n, Fq* __restrict__ out) {
  __shared__ uint4 park[12 * 64];
  __shared__ Fq sh[2][6 * 64];
  const u32 tid = threadIdx.x, pair = tid >> 1, par = lane_odd();
  Fq12 acc;
  fq12_set_one(&acc);
#pragma unroll 1
  for (u32 base = blockIdx.x * GP_PAIRS; base < n; base += gridDim.x * GP_PAIRS) {
    const u32 e = base + pair;
    const bool live = e < n;
    const Fq* src = in + (size_t)12 * (live ? e : 0u);
    fq12_mul_ld<true>(&acc, &acc, [&](int h) {      // half h of element e (2^256 form in memory) or of one
      Fq6 x;
      Fq2d* c = reinterpret_cast<Fq2d*>(&x);
#pragma unroll
      for (int k = 0; k < 3; k++) c[k].v = fq_select(live, to261(src[6 * h + 2 * k + par]), (h == 0 && k == 0) ? fq2d_one().v : fq_zero());
      return x;
    }, park);
  }
  Fq2d* c = reinterpret_cast<Fq2d*>(&acc);
  u32 buf = 0;
#pragma unroll 1
  for (u32 h = GP_PAIRS / 2; h >= 1; h >>= 1, buf ^= 1u) {
#pragma unroll
    for (int k = 0; k < 6; k++) sh[buf][k * 64 + tid] = c[k].v;
    __syncthreads();                                // one barrier a level: the next level writes the other buffer
    const Fq* src = sh[buf] + ((tid + 2 * h) & 63u);
    fq12_mul_ld<true>(&acc, &acc, [&](int hh) {
      Fq6 x;
      Fq2d* xc = reinterpret_cast<Fq2d*>(&x);
#pragma unroll
      for (int k = 0; k < 3; k++) xc[k].v = src[(3 * hh + k) * 64];
      return x;
    }, park);
  }
  if (pair == 0) {
    Fq* o = out + (size_t)12 * blockIdx.x;
#pragma unroll
    for (int k = 0; k < 6; k++) o[2 * k + par] = to256(c[k].v);
  }
}

// The pairwise mode (kzg verify_sets_each, route 2): out[i] = a[i] b[i], one lane pair per item and no tree; the same representation, the same product.
static __global__ void __launch_bounds__(64) k_gt_pair_product(const Fq* __restrict__ a, const Fq* __restrict__ b, u32 n, Fq* __restrict__ out) {
  __shared__ uint4 park[12 * 64];
  const u32 tid = threadIdx.x, par = lane_odd();
  const u32 e = blockIdx.x * GP_PAIRS + (tid >> 1);
  const bool live = e < n;
  const size_t at = (size_t)12 * (live ? e : n - 1u);       // tail pairs redo the last item and write nothing: all 64 lanes stay active
  Fq12 acc;
  Fq2d* c = reinterpret_cast<Fq2d*>(&acc);
#pragma unroll
  for (int k = 0; k < 6; k++) c[k].v = to261(a[at + 2 * k + par]);
  const Fq* src = b + at;
  fq12_mul_ld<true>(&acc, &acc, [&](int h) {
    Fq6 x;
    Fq2d* xc = reinterpret_cast<Fq2d*>(&x);
#pragma unroll
    for (int k = 0; k < 3; k++) xc[k].v = to261(src[6 * h + 2 * k + par]);
    return x;
  }, park);
  if (live) {
    Fq* o = out + at;
#pragma unroll
    for (int k = 0; k < 6; k++) o[2 * k + par] = to256(c[k].v);
  }
}

keaki_status gt_pair_product_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_b, size_t m, void* d_out) {
  if (m == 0) return KEAKI_OK;
  if (m >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "gt_pair_product: m = %zu must be < 2^31", m);
  hipLaunchKernelGGL(k_gt_pair_product, dim3(cdiv(m, GP_PAIRS)), dim3(64), 0, ctx->stream, (const Fq*)d_a, (const Fq*)d_b, (u32)m, (Fq*)d_out);
  return launch_check(ctx, "gt_pair_product");
}

size_t gt_product_part_bytes() { return (size_t)GP_MAX_BLOCKS * 12 * sizeof(Fq); }

keaki_status gt_product_run(keaki_hip_ctx* ctx, const void* d_in, size_t n, void* d_part, void* d_out) {
  if (n >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "gt_product: n = %zu must be < 2^31", n);
  if (n <= GP_ONE_BLOCK) {
    hipLaunchKernelGGL(k_gt_product, dim3(1), dim3(64), 0, ctx->stream, (const Fq*)d_in, (u32)n, (Fq*)d_out);
  } else {
    const u32 blocks = std::min<u32>(cdiv(n, GP_ONE_BLOCK), GP_MAX_BLOCKS);
    hipLaunchKernelGGL(k_gt_product, dim3(blocks), dim3(64), 0, ctx->stream, (const Fq*)d_in, (u32)n, (Fq*)d_part);
    hipLaunchKernelGGL(k_gt_product, dim3(1), dim3(64), 0, ctx->stream, (const Fq*)d_part, blocks, (Fq*)d_out);
  }
  return launch_check(ctx, "gt_product");
}

}  // namespace keaki_internal
