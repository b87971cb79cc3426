// Decides the field form of the square-root exponentiation a^((p+1)/4) (keaki_amd/csrc/fq_sqrt.hip.h, used by point_codec.hip) with a measurement:
// the same fixed-window ladder over PowU29 (nine 29-bit lazy limbs, radix 2^261, dedicated squaring stream) and over PowSat (eight saturated
// 32-bit limbs, radix 2^256, the product stream as the square), one lane per element, n = 2^20 elements, 64 lanes per workgroup as in the library.
// Both results are compared word for word (the root candidate is unique), and a sample is checked by squaring on the host side of the device
// (the kernel counts candidates whose square is the input: about half of random inputs are residues).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I keaki_amd/csrc -o bench_tools/ubench_sqrt_forms bench_tools/ubench_sqrt_forms.hip
#include "fq_sqrt.hip.h"
#include <stdio.h>
#include <vector>
using namespace bn254;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <class F>
static __device__ __noinline__ Fq pow_form(const Fq a) { return fq_pow_sqrt_exp<F>(a); }

template <class F>
__global__ void __launch_bounds__(64) k_pow(const Fq* __restrict__ in, u32 n, Fq* __restrict__ out, unsigned long long* __restrict__ residues) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fq a = in[i];
  const Fq c = pow_form<F>(a);
  out[i] = c;
  if (fq_eq(fq_sqr(c), a)) atomicAdd(residues, 1ull);
}

int main() {
  const u32 n = 1u << 20;
  std::vector<Fq> h(n);
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  for (u32 i = 0; i < n; i++)
    for (int j = 0; j < 8; j++) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      h[i].l[j] = (u32)(s >> 32);
      if (j == 7) h[i].l[j] &= 0x1fffffffu;                       // below 2^253 < p: a canonical residue
    }
  Fq *d_in, *d_a, *d_b;
  unsigned long long* d_cnt;
  CK(hipMalloc(&d_in, n * sizeof(Fq))); CK(hipMalloc(&d_a, n * sizeof(Fq))); CK(hipMalloc(&d_b, n * sizeof(Fq))); CK(hipMalloc(&d_cnt, 16));
  CK(hipMemcpy(d_in, h.data(), n * sizeof(Fq), hipMemcpyHostToDevice));
  CK(hipMemset(d_cnt, 0, 16));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float best[2] = {1e9f, 1e9f};
  for (int rep = 0; rep < 7; rep++) {
    for (int form = 0; form < 2; form++) {
      CK(hipEventRecord(e0));
      if (form == 0) hipLaunchKernelGGL((k_pow<PowU29>), dim3(n / 64), dim3(64), 0, 0, d_in, n, d_a, d_cnt);
      else hipLaunchKernelGGL((k_pow<PowSat>), dim3(n / 64), dim3(64), 0, 0, d_in, n, d_b, d_cnt + 1);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 2 && ms < best[form]) best[form] = ms;            // two warm-up rounds
    }
  }
  std::vector<Fq> a(n), b(n);
  unsigned long long cnt[2];
  CK(hipMemcpy(a.data(), d_a, n * sizeof(Fq), hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), d_b, n * sizeof(Fq), hipMemcpyDeviceToHost));
  CK(hipMemcpy(cnt, d_cnt, 16, hipMemcpyDeviceToHost));
  u32 diff = 0;
  for (u32 i = 0; i < n; i++) for (int j = 0; j < 8; j++) diff += a[i].l[j] != b[i].l[j];
  printf("a^((p+1)/4), n = 2^20, one lane per element, best of 5 launches after 2 warm-up rounds\n");
  printf("  PowU29 (29-bit lazy limbs, 2^261)  %8.3f ms  %7.1f M roots/s\n", best[0], n / best[0] / 1e3);
  printf("  PowSat (saturated words, 2^256)    %8.3f ms  %7.1f M roots/s\n", best[1], n / best[1] / 1e3);
  printf("  words that differ between the forms: %u; residues among the inputs: %llu of %u per launch (7 launches: %llu, %llu)\n", diff, cnt[0] / 7, n, cnt[0], cnt[1]);
  return diff == 0 && cnt[0] == cnt[1] ? 0 : 2;
}
