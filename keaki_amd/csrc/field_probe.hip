// Field probe (keaki_hip_selftest_field_ops): ONE shipped field function per kernel on operands chosen by the host, the raw result limbs
// back. Where the on-device self-tests (selftest.hip, selftest_u29.hip) compare one device implementation with another on canonical
// residues, this hands the verdict to the caller: tests/test_gpu_field_ops.py compares every limb with Python integers, on lazy operands at
// the bounds the streams document. Record layout and op codes: include/keaki_hip.h. Nothing is reimplemented here: every op is one call.
#include <array>

#include "pair261.hip.h"
#include "internal.h"
namespace bn254 {
namespace probe {
constexpr int SLOTS = KEAKI_FOP_SLOTS, SW = KEAKI_FOP_SLOT_WORDS, REC = SLOTS * SW;
constexpr bool is_pair(int op) { return op >= KEAKI_FOP_FIRST_PAIR; }

KDEV U29 ld_u(const u32* rec, int s) {
  U29 r;
#pragma unroll
  for (int j = 0; j < 9; j++) r.l[j] = rec[s * SW + j];
  return r;
}
KDEV Fq ld_q(const u32* rec, int s) {
  Fq r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = rec[s * SW + j];
  return r;
}
KDEV Fr ld_r(const u32* rec, int s) {
  Fr r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = rec[s * SW + j];
  return r;
}
KDEV void st_u(u32 (&o)[9], const U29& x) {
#pragma unroll
  for (int j = 0; j < 9; j++) o[j] = x.l[j];
}
template <class F>
KDEV void st_q(u32 (&o)[9], const F& x) {
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = x.l[j];
}
KDEV void st_w(u32 (&o)[9], const u32* w) {
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = w[j];
}
KDEV bool canonical(const Fq& a) {
  u32 t[8], d = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) t[j] = a.l[j];
  fp_reduce_once<FqParamsRef>(t);
#pragma unroll
  for (int j = 0; j < 8; j++) d |= t[j] ^ a.l[j];
  return d == 0;
}

template <int OP>
KDEV void run_op(const u32* rec, u32 (&o)[9]) {
  using namespace p261;
  auto U = [&](int s) { return ld_u(rec, s); };
  auto Q = [&](int s) { return ld_q(rec, s); };
  auto D = [&](int s) { return Fq2d{ld_q(rec, s)}; };
  // ---- lazy streams
  if constexpr (OP == KEAKI_FOP_U29_MUL) st_u(o, u29_mul(U(0), U(1)));
  else if constexpr (OP == KEAKI_FOP_U29_MUL_REF) st_u(o, u29_mul_ref(U(0), U(1)));
  else if constexpr (OP == KEAKI_FOP_U29_SQR) st_u(o, u29_sqr(U(0)));
  else if constexpr (OP == KEAKI_FOP_U29_SQR_REF) st_u(o, u29_sqr_ref(U(0)));
  else if constexpr (OP == KEAKI_FOP_U29_MUL2) st_u(o, u29_mul2(U(0), U(1), U(2), U(3)));
  else if constexpr (OP == KEAKI_FOP_U29_DOT3) {
    const U29 a0 = U(0), b0 = U(1), a1 = U(2), b1 = U(3), a2 = U(4), b2 = U(5);
    U29 r;
    u29_dot3_asm(r.l, a0.l, b0.l, a1.l, b1.l, a2.l, b2.l);
    st_u(o, r);
  } else if constexpr (OP == KEAKI_FOP_U29_DOT4) {
    const U29 a0 = U(0), b0 = U(1), a1 = U(2), b1 = U(3), a2 = U(4), b2 = U(5), a3 = U(6), b3 = U(7);
    U29 r;
    u29_dot4_asm(r.l, a0.l, b0.l, a1.l, b1.l, a2.l, b2.l, a3.l, b3.l);
    st_u(o, r);
  } else if constexpr (OP == KEAKI_FOP_U29_DOT6) {
    const U29 a0 = U(0), b0 = U(1), a1 = U(2), b1 = U(3), a2 = U(4), b2 = U(5), a3 = U(6), b3 = U(7), a4 = U(8), b4 = U(9), a5 = U(10), b5 = U(11);
    U29 r;
    u29_dot6_asm(r.l, a0.l, b0.l, a1.l, b1.l, a2.l, b2.l, a3.l, b3.l, a4.l, b4.l, a5.l, b5.l);
    st_u(o, r);
  } else if constexpr (OP == KEAKI_FOP_U29_CARRY) st_u(o, u29_carry(U(0)));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K2) st_u(o, u29_sub(U(0), U(1), Q29::K2));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K4) st_u(o, u29_sub(U(0), U(1), Q29::K4));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K4W) st_u(o, u29_sub(U(0), U(1), Q29::K4W));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K8) st_u(o, u29_sub(U(0), U(1), Q29::K8));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K16) st_u(o, u29_sub(U(0), U(1), Q29::K16));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K16W) st_u(o, u29_sub(U(0), U(1), Q29::K16W));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K32) st_u(o, u29_sub(U(0), U(1), Q29::K32));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K64) st_u(o, u29_sub(U(0), U(1), Q29::K64));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_K128) st_u(o, u29_sub(U(0), U(1), Q29::K128));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_RAW_K16) st_u(o, u29_sub_raw(U(0), U(1), Q29::K16));
  else if constexpr (OP == KEAKI_FOP_U29_SUB_RAW_K32) st_u(o, u29_sub_raw(U(0), U(1), Q29::K32));
  else if constexpr (OP == KEAKI_FOP_U29_SUB3) st_u(o, u29_sub3(U(0), U(1), U(2)));
  else if constexpr (OP == KEAKI_FOP_U29_MAYBE_ZERO) o[0] = u29_maybe_zero(U(0)) ? 1u : 0u;
  else if constexpr (OP == KEAKI_FOP_U29_MAYBE_ZERO34) o[0] = u29_maybe_zero34(U(0)) ? 1u : 0u;
  else if constexpr (OP == KEAKI_FOP_U29_IS_ZERO) o[0] = u29_is_zero(U(0)) ? 1u : 0u;
  else if constexpr (OP == KEAKI_FOP_U29_PACK_CANONICAL) { u32 w[8]; u29_pack_canonical(w, U(0)); st_w(o, w); }
  else if constexpr (OP == KEAKI_FOP_U29_FROM_SAT_SHIFT5) { const Fq x = Q(0); st_u(o, u29_from_sat_shift5(x.l)); }
  else if constexpr (OP == KEAKI_FOP_U29_FROM_SAT_PLAIN) { const Fq x = Q(0); st_u(o, u29_from_sat_plain(x.l)); }
  else if constexpr (OP == KEAKI_FOP_U29_FROM_FQ) st_u(o, u29_from_fq(Q(0)));
  else if constexpr (OP == KEAKI_FOP_U29_TO_FQ) st_q(o, u29_to_fq(U(0)));
  else if constexpr (OP == KEAKI_FOP_U29_TO_SAT) { u32 w[8]; u29_to_sat(w, U(0)); st_w(o, w); }
  // ---- saturated streams
  else if constexpr (OP == KEAKI_FOP_FQ_MUL) st_q(o, Q(0) * Q(1));
  else if constexpr (OP == KEAKI_FOP_FQ_SQR) st_q(o, fq_sqr(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FQ_ADD) st_q(o, Q(0) + Q(1));
  else if constexpr (OP == KEAKI_FOP_FQ_SUB) st_q(o, Q(0) - Q(1));
  else if constexpr (OP == KEAKI_FOP_FQ_NEG) st_q(o, -Q(0));
  else if constexpr (OP == KEAKI_FOP_FQ_DBL) st_q(o, fq_dbl(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FQ_HALF) st_q(o, fq_half(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FQ_REDUCE_ONCE) { Fq x = Q(0); fp_reduce_once<FqParamsRef>(x.l); st_q(o, x); }
  else if constexpr (OP == KEAKI_FOP_FQ_INV_XGCD) {
    const Fq x = Q(0);
    if (canonical(x)) st_q(o, fq_inv_xgcd(x));      // the binary GCD does not end on a multiple of p: refused, not run
    else { for (int j = 0; j < 9; j++) o[j] = 0xFFFFFFFFu; }
  } else if constexpr (OP == KEAKI_FOP_FQ_INV_SAFEGCD) st_q(o, fq_inv_safegcd(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FQ_INV_FERMAT) st_q(o, fq_inv_fermat(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FQ_INV) st_q(o, fq_inv(Q(0)));
  else if constexpr (OP == KEAKI_FOP_FR_FROM_MONT) { u32 w[8]; fp_from_mont<FrParams>(w, ld_r(rec, 0)); st_w(o, w); }
  else if constexpr (OP == KEAKI_FOP_FR_MUL) st_q(o, fp_mul<FrParams>(ld_r(rec, 0), ld_r(rec, 1)));
  else if constexpr (OP == KEAKI_FOP_FR_ADD) st_q(o, fp_add<FrParams>(ld_r(rec, 0), ld_r(rec, 1)));
  else if constexpr (OP == KEAKI_FOP_FR_SUB) st_q(o, fp_sub<FrParams>(ld_r(rec, 0), ld_r(rec, 1)));
  // ---- 2^261 form, one lane
  else if constexpr (OP == KEAKI_FOP_TO261) st_q(o, to261(Q(0)));
  else if constexpr (OP == KEAKI_FOP_TO256) st_q(o, to256(Q(0)));
  else if constexpr (OP == KEAKI_FOP_CANON_WORDS) { u32 w[8]; canon_words(w, Q(0)); st_w(o, w); }
  else if constexpr (OP == KEAKI_FOP_FQ_INV261) st_q(o, fq_inv261(Q(0)));
  // ---- lane pairs
  else if constexpr (OP == KEAKI_FOP_FQ2_MUL) st_q(o, (D(0) * D(1)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_SQR) st_q(o, fq2_sqr(D(0)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_MUL_XI) st_q(o, fq2_mul_xi(D(0)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_MUL_FQ) st_q(o, fq2_mul_fq(D(0), Q(1)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_INV) st_q(o, fq2_inv(D(0)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_CONJ) st_q(o, fq2_conj(D(0)).v);
  else if constexpr (OP == KEAKI_FOP_FQ2_NEG) st_q(o, fq2_neg(D(0)).v);
  else if constexpr (OP == KEAKI_FOP_FQ4_SQR_T0 || OP == KEAKI_FOP_FQ4_SQR_T1) {
    Fq2d t0, t1;
    fq4_sqr(&t0, &t1, D(0), D(1));
    st_q(o, OP == KEAKI_FOP_FQ4_SQR_T0 ? t0.v : t1.v);
  } else if constexpr (OP == KEAKI_FOP_FQ6_MUL_C0 || OP == KEAKI_FOP_FQ6_MUL_C1 || OP == KEAKI_FOP_FQ6_MUL_C2) {
    const Fq6 a = {D(0), D(1), D(2)}, b = {D(3), D(4), D(5)};
    Fq6 r;
    fq6_mul(&r, &a, &b);
    st_q(o, OP == KEAKI_FOP_FQ6_MUL_C0 ? r.c0.v : OP == KEAKI_FOP_FQ6_MUL_C1 ? r.c1.v : r.c2.v);
  } else static_assert(OP < 0, "field probe: op without a body");
}

// one record per lane. Lane-pair ops: the DPP moves of pair261.hip.h need all 64 lanes, so the launch covers whole waves of records (the
// host pads `in`), nobody returns early and only the store is guarded.
template <int OP>
__global__ void __launch_bounds__(64) k_field_probe(const u32* __restrict__ in, u32 n, u32* __restrict__ out) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if constexpr (!is_pair(OP)) {
    if (i >= n) return;
  }
  u32 o[9];
#pragma unroll
  for (int j = 0; j < 9; j++) o[j] = 0;
  run_op<OP>(in + (size_t)i * REC, o);
  if (i < n) {
#pragma unroll
    for (int j = 0; j < 9; j++) out[(size_t)i * SW + j] = o[j];
  }
}

typedef void (*Launch)(hipStream_t, const u32*, u32, u32, u32*);
template <int OP>
void launch(hipStream_t s, const u32* in, u32 n, u32 blocks, u32* out) {
  hipLaunchKernelGGL((k_field_probe<OP>), dim3(blocks), dim3(64), 0, s, in, n, out);
}
template <int... OPS>
constexpr std::array<Launch, sizeof...(OPS)> make_table(std::integer_sequence<int, OPS...>) { return {{&launch<OPS>...}}; }
static const auto TABLE = make_table(std::make_integer_sequence<int, KEAKI_FOP_COUNT>{});
}  // namespace probe
}  // namespace bn254

namespace keaki_internal {
bool field_probe_is_pair(uint32_t op) { return bn254::probe::is_pair((int)op); }
size_t field_probe_padded(uint32_t op, size_t n) { return field_probe_is_pair(op) ? (n + 63) / 64 * 64 : n; }
keaki_status field_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out) {
  if (op >= KEAKI_FOP_COUNT || n == 0 || n > KEAKI_FOP_MAX_RECORDS || !d_operands || !d_out || (field_probe_is_pair(op) && (n & 1)))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "field_probe: bad argument");
  bn254::probe::TABLE[op](ctx->stream, (const uint32_t*)d_operands, (uint32_t)n, cdiv(n, 64), (uint32_t*)d_out);
  return launch_check(ctx, "field_probe");
}
}  // namespace keaki_internal
