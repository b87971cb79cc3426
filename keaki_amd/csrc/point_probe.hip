// Point probe (keaki_hip_selftest_point_ops), G1 half: ONE shipped function of the lazy-limb group law (xyzz29.hip.h, jac29.hip.h), of the GLV
// code, of the four ladders or of the saturated formulas over Fq (bn254_curve.hip.h) per kernel, on operands chosen by the host; raw limbs,
// words, flags and return values back. The on-device self-tests (k_selftest_x29, k_selftest_j29) compare the lazy code with the same compiler's
// saturated code on canonical residues drawn on the device and return a count; here the host places every limb -- coordinates at the bounds the
// headers document, every multiple of p a zero test can meet, scalars at the rounding steps and carry chains of the GLV code -- and Python
// integers judge the result (tests/point_ref.py, tests/test_gpu_point_ops.py). Record layout, op codes and what is NOT probed (the inline mixed
// addition of k_msm_accumulate_g1_u29, fb_accumulate*, the Straus kernels of fk_coset.hip and vec_update.hip, the branch "u29_maybe_zero fires,
// u29_is_zero does not"): include/keaki_hip.h. Nothing is reimplemented here: every op is one call with the template arguments of a shipped
// call site (the two-term ladder builds its tables with j29_build_pair first, as fft_g1.hip does). The G2 half: point_probe_g2.hip.
#include <array>

#include "point_probe.hip.h"
#include "xyzz29.hip.h"
#include "jac29.hip.h"
namespace bn254 {
namespace pprobe {
KDEV X29 ld_x29(const u32* rec, int s, int flag) { return {ld_u(rec, s), ld_u(rec, s + 1), ld_u(rec, s + 2), ld_u(rec, s + 3), rec[FLAGS + flag]}; }
KDEV void st_x29(u32* o, const X29& p) {
  st_u(o, 0, p.x); st_u(o, 1, p.y); st_u(o, 2, p.zz); st_u(o, 3, p.zzz);
  o[OFLAGS] = p.inf;
}
KDEV J29 ld_j29(const u32* rec, int s) { return {ld_u(rec, s), ld_u(rec, s + 1), ld_u(rec, s + 2)}; }
KDEV void st_j29(u32* o, int s, const J29& p) { st_u(o, s, p.x); st_u(o, s + 1, p.y); st_u(o, s + 2, p.z); }
KDEV void st_table(u32* o, int s, const J29A* T) {
#pragma unroll 1
  for (int e = 0; e < 8; e++) { st_u(o, s + 3 * e, T[e].x); st_u(o, s + 3 * e + 1, T[e].xb); st_u(o, s + 3 * e + 2, T[e].y); }
}

// dig: this wave's 4 x UNIFORM_DIG_STRIDE bytes of LDS; tab: this lane's 1 KB of the table workspace (KEAKI_POP_LADDER_GTAB only)
template <int OP>
KDEV void run_op(const u32* rec, u32* o, unsigned char* dig, uint4* tab) {
  if constexpr (OP == KEAKI_POP_X29_ADD) st_x29(o, x29_add(ld_x29(rec, 0, 0), ld_x29(rec, 4, 1)));
  else if constexpr (OP == KEAKI_POP_X29_DBL) st_x29(o, x29_dbl(ld_x29(rec, 0, 0)));
  else if constexpr (OP == KEAKI_POP_X29_STORE) st_xyzz(o, x29_store(ld_x29(rec, 0, 0)));
  else if constexpr (OP == KEAKI_POP_X29_LOAD_STORE) st_xyzz(o, x29_store(x29_load(ld_xyzz<Fq>(rec, 0))));
  else if constexpr (OP == KEAKI_POP_J29_DBL) st_j29(o, 0, j29_dbl(ld_j29(rec, 0)));
  else if constexpr (OP == KEAKI_POP_J29_MADD) {
    int special;
    U29 ratio;
#pragma unroll
    for (int j = 0; j < 9; j++) ratio.l[j] = 0;
    st_j29(o, 0, j29_madd(ld_j29(rec, 0), ld_u(rec, 3), ld_u(rec, 4), special, &ratio));
    st_u(o, 3, ratio);
    o[OFLAGS] = (u32)special;
  } else if constexpr (OP == KEAKI_POP_J29_ADDSUB) {
    J29 sum, diff;
#pragma unroll
    for (int j = 0; j < 9; j++) sum.x.l[j] = sum.y.l[j] = sum.z.l[j] = diff.x.l[j] = diff.y.l[j] = diff.z.l[j] = 0;
    const bool ok = j29_addsub(ld_j29(rec, 0), ld_j29(rec, 3), sum, diff);
    st_j29(o, 0, sum); st_j29(o, 3, diff);
    o[OFLAGS] = ok ? 1u : 0u;
  } else if constexpr (OP == KEAKI_POP_J29_SAT_ROUNDTRIP) st_jac(o, j29_to_sat(j29_from_sat(ld_jac<Fq>(rec, 0))));
  else if constexpr (OP == KEAKI_POP_J29_BUILD_TABLE || OP == KEAKI_POP_J29_BUILD_TABLE_ODD) {
    J29A T[8];
    J29ArrTable tb = {T, u29_const(GlvParams::BETA29)};
    const U29 zfix = j29_build_table<OP == KEAKI_POP_J29_BUILD_TABLE_ODD>(ld_jac<Fq>(rec, 0), tb);
    st_table(o, 0, T);
    st_u(o, 24, zfix);
  } else if constexpr (OP == KEAKI_POP_J29_BUILD_PAIR) {
    J29A T[16];
    J29PairTables t = {T, T + 8, {}};
    j29_build_pair(ld_jac<Fq>(rec, 0), ld_jac<Fq>(rec, 3), t);
    st_table(o, 0, t.TA); st_table(o, 24, t.TB);
    st_u(o, 48, t.zfix);
  } else if constexpr (OP == KEAKI_POP_GLV_DECOMPOSE) {
    u32 k[8], k1[5], k2[5];
    bool neg1, neg2;
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = rec[j];
    glv_decompose(k, k1, neg1, k2, neg2);
#pragma unroll
    for (int j = 0; j < 5; j++) { o[j] = k1[j]; o[SW + j] = k2[j]; }
    o[OFLAGS] = neg1 ? 1u : 0u; o[OFLAGS + 1] = neg2 ? 1u : 0u;
  } else if constexpr (OP == KEAKI_POP_GLV_FIXED_DIGITS) {
    u32 k[5], d[5], sg[2];
#pragma unroll
    for (int j = 0; j < 5; j++) k[j] = rec[j];
    glv_fixed_digits(k, d, sg);
#pragma unroll
    for (int j = 0; j < 5; j++) o[j] = d[j];
    o[SW] = sg[0]; o[SW + 1] = sg[1];
  } else if constexpr (OP == KEAKI_POP_GLV_UNIFORM_DIGITS) {
    bool neg1, neg2;
    glv_uniform_digits(ld_w<Fr>(rec, 0), dig, neg1, neg2);
    __syncthreads();
#pragma unroll 1
    for (int w = 0; w < 2 * UNIFORM_DIG_STRIDE / 4; w++)
      o[w] = (u32)dig[4 * w] | ((u32)dig[4 * w + 1] << 8) | ((u32)dig[4 * w + 2] << 16) | ((u32)dig[4 * w + 3] << 24);
    o[OFLAGS] = neg1 ? 1u : 0u; o[OFLAGS + 1] = neg2 ? 1u : 0u;
  } else if constexpr (OP == KEAKI_POP_LADDER_FIXED || OP == KEAKI_POP_LADDER_GTAB || OP == KEAKI_POP_LADDER_UNIFORM) {
    J29 r;
#pragma unroll
    for (int j = 0; j < 9; j++) r.x.l[j] = r.y.l[j] = r.z.l[j] = 0;
    const Jac<Fq> p = ld_jac<Fq>(rec, 0);
    const Fr k = ld_w<Fr>(rec, 3);
    bool ok;
    if constexpr (OP == KEAKI_POP_LADDER_FIXED) ok = jac_scalar_mul_u29_j(p, k, r);
    else if constexpr (OP == KEAKI_POP_LADDER_GTAB) ok = jac_scalar_mul_gtab_u29_j(p, k, tab, r);
    else ok = jac_scalar_mul_uniform_u29_j(p, k, dig, r);
    st_j29(o, 0, r);
    o[OFLAGS] = ok ? 1u : 0u;
  } else if constexpr (OP == KEAKI_POP_LADDER_MUL2) {
    J29A T[16];
    J29PairTables t = {T, T + 8, {}};
    j29_build_pair(ld_jac<Fq>(rec, 0), ld_jac<Fq>(rec, 3), t);
    J29 r;
#pragma unroll
    for (int j = 0; j < 9; j++) r.x.l[j] = r.y.l[j] = r.z.l[j] = 0;
    const bool negB = __builtin_amdgcn_readfirstlane((int)rec[FLAGS + 2]) != 0;
    const bool ok = j29_mul2_uniform(t, ld_w<Fr>(rec, 6), ld_w<Fr>(rec, 7), negB, dig, r);
    st_j29(o, 0, r);
    o[OFLAGS] = ok ? 1u : 0u;
  } else if constexpr (OP >= KEAKI_POP_XYZZ_ADD_MIXED_FQ && OP <= KEAKI_POP_JAC_DBL_FQ) run_sat<Fq, OP - KEAKI_POP_XYZZ_ADD_MIXED_FQ>(rec, o);
  else static_assert(OP < 0, "point probe: op without a body");
}

// one record per lane, whole waves (the host pads `in`, and `out` has a record for every lane that runs: nobody returns early, the wave-uniform
// forms need their first lane whatever n is)
template <int OP>
__global__ void __launch_bounds__(64) k_point_probe(const u32* __restrict__ in, u32* __restrict__ out, uint4* __restrict__ tab) {
  __shared__ unsigned char dig[4 * UNIFORM_DIG_STRIDE];
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  run_op<OP>(in + (size_t)i * REC, out + (size_t)i * OUT, dig, tab ? tab + (size_t)i * GTAB_UINT4_PER_LANE : nullptr);
}
template <int OP>
void launch(hipStream_t s, const u32* in, u32 n, u32 blocks, u32* out, uint4* tab) {
  hipLaunchKernelGGL((k_point_probe<OP>), dim3(blocks), dim3(64), 0, s, in, out, tab);
}
template <int... OPS>
constexpr std::array<Launch, sizeof...(OPS)> make_table(std::integer_sequence<int, OPS...>) { return {{&launch<OPS>...}}; }
static const auto TABLE = make_table(std::make_integer_sequence<int, KEAKI_POP_FIRST_G2>{});
}  // namespace pprobe
}  // namespace bn254

namespace keaki_internal {
size_t point_probe_padded(size_t n) { return (n + 63) / 64 * 64; }
size_t point_probe_table_bytes(uint32_t op, size_t n) {
  return op == KEAKI_POP_LADDER_GTAB ? point_probe_padded(n) * bn254::GTAB_UINT4_PER_LANE * sizeof(uint4) : 0;
}
keaki_status point_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out, void* d_table) {
  if (op >= KEAKI_POP_COUNT || n == 0 || n > KEAKI_POP_MAX_RECORDS || !d_operands || !d_out || (op == KEAKI_POP_LADDER_GTAB && !d_table))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "point_probe: bad argument");
  const uint32_t blocks = (uint32_t)(point_probe_padded(n) / 64);
  if (op >= KEAKI_POP_FIRST_G2) point_probe_g2_launch(ctx->stream, op - KEAKI_POP_FIRST_G2, (const uint32_t*)d_operands, (uint32_t)n, blocks, (uint32_t*)d_out);
  else bn254::pprobe::TABLE[op](ctx->stream, (const uint32_t*)d_operands, (uint32_t)n, blocks, (uint32_t*)d_out, (uint4*)d_table);
  return launch_check(ctx, "point_probe");
}
}  // namespace keaki_internal
