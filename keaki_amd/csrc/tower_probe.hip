// Tower probe (keaki_hip_selftest_tower_ops), lane-pair form: ONE shipped function of the pairing's Fq12 tower per kernel on operands chosen by the
// host, all twelve result words back. The field probe (field_probe.hip) hands the caller every Fq-level stream up to fq6_mul; this one does the
// same for what stands on them: the Fq12 operations of pair261.hip.h and the line functions of pairing.hip.h, which the suite otherwise sees
// only from the far end of a pairing, where every coefficient is uniform mod p. tests/test_gpu_tower_ops.py compares every word with Python
// integers (tests/tower_ref.py). Record layout, op codes and what is NOT probed: include/keaki_hip.h. Nothing is reimplemented here: every op is
// one call, with the template arguments, the aliasing and the parking indices of a shipped call site (k_pairing, k_pairing2, k_gt_table_fill,
// k_gt_encap_exp; fq12_inv<false> is w12_inv's). The twelve-lane form: tower_probe_wide.hip.
#define KEAKI_FQ2_OUTLINE 1
#include "tower_probe.hip.h"
namespace bn254 {
namespace tprobe {

// this lane's components of an Fq12 (Fq2 coefficient m at Fq 2m + parity), of the running point and of the affine point
KDEV void ld_f12(Fq12* f, const u32* rec, int off) {
  Fq2d* c = reinterpret_cast<Fq2d*>(f);
  const u32 par = lane_odd();
#pragma unroll
  for (int m = 0; m < 6; m++) c[m].v = ld_fq(rec, off, 2u * m + par);
}
KDEV void st_f12(u32* out, const Fq12* f) {
  const Fq2d* c = reinterpret_cast<const Fq2d*>(f);
  const u32 par = lane_odd();
#pragma unroll
  for (int m = 0; m < 6; m++) st_fq(out, 2u * m + par, c[m].v);
}

// `arg`: the Frobenius power (a run-time value in fe_run too)
template <int OP>
KDEV void run_op(const u32* rec, int arg, uint4* park, Fq12* r) {
  const u32 par = lane_odd();
  if constexpr (OP == KEAKI_TOP_LINE_DOUBLE || OP == KEAKI_TOP_LINE_ADD) {
    G2Hom t = {{ld_fq(rec, T_OFF, par)}, {ld_fq(rec, T_OFF, 2u + par)}, {ld_fq(rec, T_OFF, 4u + par)}};
    Line l;
    if constexpr (OP == KEAKI_TOP_LINE_DOUBLE) {
      line_double(&t, &l);
    } else {
      const Fq2d qx = {ld_fq(rec, Q_OFF, par)}, qy = {ld_fq(rec, Q_OFF, 2u + par)};
      line_add(&t, &qx, &qy, &l);
    }
    r->c0 = {t.x, t.y, t.z};
    r->c1 = {l.c0, l.c1, l.c2};
  } else if constexpr (OP == KEAKI_TOP_FQ6_INV) {
    const Fq6 a = {{ld_fq(rec, A_OFF, par)}, {ld_fq(rec, A_OFF, 2u + par)}, {ld_fq(rec, A_OFF, 4u + par)}};
    fq6_inv(&r->c0, &a);
    r->c1 = fq6_zero();
  } else {
    ld_f12(r, rec, A_OFF);
    if constexpr (OP == KEAKI_TOP_FQ12_MUL) {
      Fq12 b;
      ld_f12(&b, rec, B_OFF);
      fq12_mul(r, r, &b);
    } else if constexpr (OP == KEAKI_TOP_FQ12_MUL_LD) {
      fq12_mul_ld<true>(r, r, [&](int h) {
        Fq6 x;
        Fq2d* c = reinterpret_cast<Fq2d*>(&x);
#pragma unroll
        for (int k = 0; k < 3; k++) c[k].v = ld_fq(rec, B_OFF, 6u * h + 2u * k + par);
        return x;
      }, park);
    } else if constexpr (OP == KEAKI_TOP_FQ12_SQR) fq12_sqr<true>(r, r, park, 3);
    else if constexpr (OP == KEAKI_TOP_FQ12_INV) { Fq12 a = *r; fq12_inv<false>(r, &a); }
    else if constexpr (OP == KEAKI_TOP_FQ12_INV_PARKED) fq12_inv<true>(r, r, park);
    else if constexpr (OP == KEAKI_TOP_FQ12_CONJ) fq12_conj(r, r);
    else if constexpr (OP == KEAKI_TOP_FQ12_CYC_SQR) fq12_cyc_sqr<true>(r, r, park);
    else if constexpr (OP == KEAKI_TOP_FQ12_FROB1) fq12_frob(r, r, arg);
    else if constexpr (OP == KEAKI_TOP_FQ12_FROB_PARKED1) fq12_frob_parked(r, r, arg, park);
    else if constexpr (OP == KEAKI_TOP_FQ12_MUL_BY_034)
      fq12_mul_by_034_limbs<true>(r, ld_limbs(rec, LINE_OFF, par), ld_limbs(rec, LINE_OFF, 2u + par), ld_limbs(rec, LINE_OFF, 4u + par), true, park, 3);
    else if constexpr (OP == KEAKI_TOP_ELL) {
      const Line l = {{ld_fq(rec, T_OFF, par)}, {ld_fq(rec, T_OFF, 2u + par)}, {ld_fq(rec, T_OFF, 4u + par)}};
      ell(r, &l, ld_limbs(rec, P_OFF, 0), ld_limbs(rec, P_OFF, 1), park, 3);
    } else static_assert(OP < 0, "tower probe: op without a body");
  }
}

// one record per lane pair. The DPP moves of pair261.hip.h need all 64 lanes: the launch covers whole waves of records (the host pads `in`),
// nobody returns early and only the store is guarded. LDS: k_pairing's parking area.
template <int OP>
__global__ void __launch_bounds__(64, 2) k_tower_probe(const u32* __restrict__ in, u32 n, u32* __restrict__ out, int arg) {
  __shared__ uint4 park[PARK_CHUNKS * 64 + 16];
  const u32 i = (blockIdx.x * 64u + threadIdx.x) >> 1;
  Fq12 r;
  run_op<OP>(in + (size_t)i * REC, arg, park, &r);
  if (i < n) st_f12(out + (size_t)i * OUT, &r);
}
template <int OP>
void launch(hipStream_t s, const u32* in, u32 n, u32 blocks, u32* out, int arg) {
  hipLaunchKernelGGL((k_tower_probe<OP>), dim3(blocks), dim3(64), 0, s, in, n, out, arg);
}
#define E(op) {&launch<KEAKI_TOP_##op>, 0}
static const Entry TABLE[KEAKI_TOP_FIRST_WIDE] = {
  E(FQ12_MUL), E(FQ12_MUL_LD), E(FQ12_SQR), E(FQ12_INV), E(FQ12_INV_PARKED), E(FQ12_CONJ), E(FQ12_CYC_SQR),
  {&launch<KEAKI_TOP_FQ12_FROB1>, 1}, {&launch<KEAKI_TOP_FQ12_FROB1>, 2}, {&launch<KEAKI_TOP_FQ12_FROB1>, 3},
  {&launch<KEAKI_TOP_FQ12_FROB_PARKED1>, 1}, {&launch<KEAKI_TOP_FQ12_FROB_PARKED1>, 2}, {&launch<KEAKI_TOP_FQ12_FROB_PARKED1>, 3},
  E(FQ12_MUL_BY_034), E(ELL), E(FQ6_INV), E(LINE_DOUBLE), E(LINE_ADD),
};
#undef E
static_assert(KEAKI_TOP_FQ12_MUL == 0 && KEAKI_TOP_FQ12_FROB1 == 7 && KEAKI_TOP_FQ12_FROB_PARKED1 == 10 && KEAKI_TOP_FQ12_MUL_BY_034 == 13 &&
              KEAKI_TOP_LINE_ADD == 17 && KEAKI_TOP_FIRST_WIDE == 18, "tower probe: the table follows the enum");
}  // namespace tprobe
}  // namespace bn254

namespace keaki_internal {
bool tower_probe_is_wide(uint32_t op) { return op >= KEAKI_TOP_FIRST_WIDE; }
size_t tower_probe_padded(uint32_t op, size_t n) { const size_t per = tower_probe_is_wide(op) ? 4 : 32; return (n + per - 1) / per * per; }
keaki_status tower_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out) {
  if (op >= KEAKI_TOP_COUNT || n == 0 || n > KEAKI_TOP_MAX_RECORDS || !d_operands || !d_out) return fail(ctx, KEAKI_ERR_BAD_ARG, "tower_probe: bad argument");
  const uint32_t blocks = (uint32_t)(tower_probe_padded(op, n) / (tower_probe_is_wide(op) ? 4 : 32));
  if (tower_probe_is_wide(op)) {
    tower_probe_wide_launch(ctx->stream, op - KEAKI_TOP_FIRST_WIDE, (const uint32_t*)d_operands, (uint32_t)n, blocks, (uint32_t*)d_out);
  } else {
    const bn254::tprobe::Entry& e = bn254::tprobe::TABLE[op];
    e.launch(ctx->stream, (const uint32_t*)d_operands, (uint32_t)n, blocks, (uint32_t*)d_out, e.arg);
  }
  return launch_check(ctx, "tower_probe");
}
}  // namespace keaki_internal
