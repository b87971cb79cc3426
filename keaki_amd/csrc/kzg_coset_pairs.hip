// KZG coset pairs (keaki_hip_kzg_coset_pairs): the group side. For item k (a coset h_k <omega_l> with l claimed values) the call returns
//     A_k = C_k - [I_k(tau)]_1 = C_k + sum_j (-a_(k,j)) [tau^j]_1        c_k = h_k^l
// the two per-item inputs of the coset check e(A_k, g2) == e(proof_k, [tau^l]_2 - c_k g2). The Fr side (kzg_cosets.hip: k_vc_prepare<., true>,
// k_vc_transform<., true>) leaves c_k and, per launch chunk, the rows -a_(k,j) in (item, j) order, 32 B each. What lives here:
//   k_cp_rows     route 1. All rows share the l bases [tau^j]_1, so the handle keeps a window table T[j][w][d] = d 2^(wb w) [tau^j]_1 (ec_batch_g1.hip:
//                 g1_fb_tables_run; wb from coset_rows_plan.h) and a row costs l x windows additions and no doublings. A lane owns one (item, slice of
//                 the l bases): it walks the signed wb-bit digits of each of its scalars exactly as fb_accumulate does (carry into the next digit
//                 included) and adds the table entries to an accumulator in the lazy 29-bit XYZZ form (xyzz29.hip.h). x29_add is the complete
//                 addition: equal operands double, opposite ones give the identity and the walk goes on, an identity entry (an SRS point (0,0)) is
//                 skipped. The S slices of an item sit in neighbouring lanes of one wave and meet in log2 S rounds of cross-lane exchange (37 words a
//                 round) with the same addition; lane 0 of the item adds C_k (which may be the identity) and stores the sum in XYZZ.
//   k_cp_join     route 2. The rows went through msm_g1_batch_run as Montgomery scalars; this adds C_k to the Jacobian sums, into the same XYZZ slots.
//   k_cp_affine   XYZZ -> affine with (0,0) for the identity, CP_INV = 8 items per lane under ONE inversion (Montgomery's trick over the zzz): at l = 4
//                 a row is 80 additions, against which one inversion per item would be a third of the call.
// Both routes end in the unique affine form, so they agree to the byte.
#include "ec_batch.hip.h"
#include "xyzz29.hip.h"
#include "internal.h"
namespace keaki_internal {
using namespace bn254;

constexpr u32 CP_INV = 8;

KDEV U29 cp_shfl_xor(const U29& a, u32 mask) {
  U29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (u32)__shfl_xor((int)a.l[i], (int)mask, 64);
  return r;
}
KDEV X29 cp_shfl_xor(const X29& a, u32 mask) {
  X29 r;
  r.x = cp_shfl_xor(a.x, mask); r.y = cp_shfl_xor(a.y, mask); r.zz = cp_shfl_xor(a.zz, mask); r.zzz = cp_shfl_xor(a.zzz, mask);
  r.inf = (u32)__shfl_xor((int)a.inf, (int)mask, 64);
  return r;
}

// lane = item * S + slice over the m items of a chunk; S = 2^log2S <= min(l, 64) divides the wave, so an item never straddles two waves. Lanes past
// m * S redo the last item (the exchange needs every lane of a wave) and store nothing.
static __global__ void __launch_bounds__(64) k_cp_rows(const G1Aff* __restrict__ table, FbShape g, const u32* __restrict__ rows, u32 log2l, u32 log2S,
                                                       const G1Aff* __restrict__ coms, u32 com_stride, u32 m, G1Xyzz* __restrict__ out) {
  const u32 lane = blockIdx.x * 64u + threadIdx.x;
  const u32 item = lane >> log2S, slice = lane & ((1u << log2S) - 1u);
  const bool live = item < m;
  const u32 k = live ? item : m - 1u;
  const u32 per = 1u << (log2l - log2S), half = 1u << (g.wb - 1);
  const size_t per_base = (size_t)g.windows * g.entries;
  X29 acc = x29_inf();
#pragma unroll 1
  for (u32 j = slice * per; j < (slice + 1u) * per; j++) {
    const uint4* src = reinterpret_cast<const uint4*>(rows + (((size_t)k << log2l) + j) * 8u);
    const uint4 lo = src[0], hi = src[1];
    u32 v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const G1Aff* tab = table + (size_t)j * per_base;
    u32 carry = 0;
#pragma unroll 1
    for (u32 w = 0; w < g.windows; w++) {
      u32 d = (v[0] & (2u * half - 1u)) + carry;
#pragma unroll
      for (int t = 0; t < 7; t++) v[t] = (v[t] >> g.wb) | (v[t + 1] << (32u - g.wb));
      v[7] >>= g.wb;
      const bool neg = d > half;                       // d - 2^wb and a carry (2^wb itself: digit 0, carry 1)
      carry = neg ? 1u : 0u;
      if (neg) d = 2u * half - d;
      if (d) acc = x29_add(acc, x29_load(xyzz_from_aff(aff_cneg(tab[(size_t)w * g.entries + d], neg))));
    }
  }
#pragma unroll 1
  for (u32 step = 1; step < (1u << log2S); step <<= 1) acc = x29_add(acc, cp_shfl_xor(acc, step));   // every lane adds; slice 0 holds the item's sum
  if (!live || slice) return;
  const G1Aff c = coms[(size_t)item * com_stride];
  acc = x29_add(acc, x29_load(xyzz_from_aff(c)));
  out[item] = x29_store(acc);
}

static __global__ void __launch_bounds__(64) k_cp_join(const G1Jac* __restrict__ sums, const G1Aff* __restrict__ coms, u32 com_stride, u32 m,
                                                       G1Xyzz* __restrict__ out) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= m) return;
  const G1Jac a = jac_add(jac_from_aff(coms[(size_t)i * com_stride]), sums[i]);
  G1Xyzz r = xyzz_inf<Fq>();
  if (!jac_is_inf(a)) {
    const Fq zz = f_sqr(a.z);
    r = {a.x, a.y, zz, zz * a.z};
  }
  out[i] = r;
}

static __global__ void __launch_bounds__(64) k_cp_affine(const G1Xyzz* __restrict__ in, u32 m, G1Aff* __restrict__ out) {
  const u32 k0 = (blockIdx.x * 64u + threadIdx.x) * CP_INV;
  if (k0 >= m) return;
  Fq pre[CP_INV];                                    // pre[i] = zzz_k0 .. zzz_(k0 + i), an identity or a slot past m counting as one
  Fq run = f_one<Fq>();
#pragma unroll
  for (u32 i = 0; i < CP_INV; i++) {
    if (k0 + i < m) {
      const Fq zzz = in[k0 + i].zzz;
      if (!f_is_zero(zzz)) run = run * zzz;
    }
    pre[i] = run;
  }
  Fq inv = f_inv(run);
#pragma unroll
  for (u32 t = 0; t < CP_INV; t++) {
    const u32 i = CP_INV - 1u - t;                   // a compile-time index after unrolling: pre[] stays in registers
    if (k0 + i < m) {
      const G1Xyzz p = in[k0 + i];
      G1Aff r = aff_inf<Fq>();
      if (!f_is_zero(p.zz)) {
        const Fq izzz = i ? inv * pre[i ? i - 1u : 0u] : inv;
        inv = inv * p.zzz;
        const Fq izz = f_sqr(izzz) * f_sqr(p.zz);    // zz^-1 = zzz^-2 zz^2 (zz^3 = zzz^2)
        r = {p.x * izz, p.y * izzz};
      }
      out[k0 + i] = r;
    }
  }
}

keaki_status coset_table_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2l, uint32_t wb, void* d_table) {
  return g1_fb_tables_run(ctx, d_srs, 1u << log2l, d_table, wb);
}

keaki_status coset_rows_table_run(keaki_hip_ctx* ctx, const void* d_table, uint32_t wb, const void* d_rows, uint32_t log2l, uint32_t S, const void* d_coms,
                                  int com_stride, size_t first, size_t m, void* d_xyzz) {
  u32 log2S = 0;
  while ((1u << log2S) < S) log2S++;
  if (m == 0 || (1u << log2S) != S || log2S > 6 || log2S > log2l || (m << log2l) >= ((size_t)1 << 31))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_coset_pairs: a chunk of %zu items of 2^%u values in %u slices out of range on the device side", m, log2l, S);
  const G1Aff* coms = (const G1Aff*)d_coms + (com_stride ? first : 0);
  hipLaunchKernelGGL(k_cp_rows, dim3(cdiv(m << log2S, 64)), dim3(64), 0, ctx->stream, (const G1Aff*)d_table, fb_shape(wb), (const u32*)d_rows, log2l, log2S, coms,
                     (u32)com_stride, (u32)m, (G1Xyzz*)d_xyzz);
  return launch_check(ctx, "coset_rows");
}

keaki_status coset_rows_join_run(keaki_hip_ctx* ctx, const void* d_sums_jac, const void* d_coms, int com_stride, size_t first, size_t m, void* d_xyzz) {
  if (m == 0) return KEAKI_OK;
  const G1Aff* coms = (const G1Aff*)d_coms + (com_stride ? first : 0);
  hipLaunchKernelGGL(k_cp_join, dim3(cdiv(m, 64)), dim3(64), 0, ctx->stream, (const G1Jac*)d_sums_jac, coms, (u32)com_stride, (u32)m, (G1Xyzz*)d_xyzz);
  return launch_check(ctx, "coset_rows_join");
}

keaki_status coset_rows_affine_run(keaki_hip_ctx* ctx, const void* d_xyzz, size_t m, void* d_out_aff) {
  if (m == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_cp_affine, dim3(cdiv(cdiv(m, CP_INV), 64)), dim3(64), 0, ctx->stream, (const G1Xyzz*)d_xyzz, (u32)m, (G1Aff*)d_out_aff);
  return launch_check(ctx, "coset_rows_affine");
}

}  // namespace keaki_internal
