// Tower probe (keaki_hip_selftest_tower_ops), twelve-lane form: ONE function of pairing_wide.hip.h per kernel on operands chosen by the host. That
// form has product code of its own -- the schoolbook sum over six pairs with the wrapped terms picked by ADDRESS in the exchange area, the line
// forms chosen per pair, the Granger-Scott squaring with its special case for pair 1 -- and a wrong wrap in one pair changes a result only on
// operands a random pairing never holds. Geometry as k_pairing_wide: one record per 16-lane row, four per wave; pair k of a row loads and stores
// the flat coefficient of w^k, which sits at Fq2 position m = (k & 1) * 3 + (k >> 1) of the tower's memory order; lanes 12..15 shadow pairs 0
// and 1 and store nothing. Layout and op codes: include/keaki_hip.h; the lane-pair form and the host entry: tower_probe.hip.
#define KEAKI_FQ2_OUTLINE 1
#include "tower_probe.hip.h"
namespace bn254 {
namespace tprobe {
using namespace pw;

template <int OP>
KDEV Fq run_wide(const u32* rec, int arg, uint4* ex) {
  const u32 par = lane_odd(), k = my_pair(), m = (k & 1u) * 3u + (k >> 1);
  if constexpr (OP == KEAKI_TOP_W_LINE_DOUBLE || OP == KEAKI_TOP_W_LINE_ADD) {
    // T (and Q) replicated in every pair, as in w_miller; pair k reports Fq2 number k of (X', Y', Z', c0, c1, c2)
    G2Hom t = {{ld_fq(rec, T_OFF, par)}, {ld_fq(rec, T_OFF, 2u + par)}, {ld_fq(rec, T_OFF, 4u + par)}};
    Line l;
    if constexpr (OP == KEAKI_TOP_W_LINE_DOUBLE) {
      w_line_double(&t, &l, ex);
    } else {
      const Fq2d qx = {ld_fq(rec, Q_OFF, par)}, qy = {ld_fq(rec, Q_OFF, 2u + par)};
      w_line_add(&t, qx, qy, &l, ex);
    }
    return pick6(k, t.x, t.y, t.z, l.c0, l.c1, l.c2).v;
  } else {
    const Fq a = ld_fq(rec, A_OFF, 2u * m + par);
    if constexpr (OP == KEAKI_TOP_W12_MUL) return w12_mul(a, ld_fq(rec, B_OFF, 2u * m + par), ex);
    else if constexpr (OP == KEAKI_TOP_W12_MUL_034)
      return w12_mul_034(a, ld_limbs(rec, LINE_OFF, par), ld_limbs(rec, LINE_OFF, 2u + par), ld_limbs(rec, LINE_OFF, 4u + par), ex);
    else if constexpr (OP == KEAKI_TOP_W12_CYC_SQR) return w12_cyc_sqr(a, ex);
    else if constexpr (OP == KEAKI_TOP_W12_FROB1) return w12_frob(a, arg);
    else if constexpr (OP == KEAKI_TOP_W12_CONJ) return w12_conj(a);
    else if constexpr (OP == KEAKI_TOP_W12_INV) return w12_inv(a, ex);
    else if constexpr (OP == KEAKI_TOP_W12_GATHER_OWN) { Fq12 f; w12_gather(&f, a, ex); return w12_own(&f); }
    else static_assert(OP < 0, "tower probe: wide op without a body");
  }
}

// All 64 lanes run (DPP exchanges, and every pair of a row publishes to the exchange area): the host pads `in` to whole waves of four records.
template <int OP>
__global__ void __launch_bounds__(64) k_tower_probe_wide(const u32* __restrict__ in, u32 n, u32* __restrict__ out, int arg) {
  __shared__ uint4 ex[EX_UINT4];
  const u32 i = blockIdx.x * 4u + (threadIdx.x >> 4);
  const Fq r = run_wide<OP>(in + (size_t)i * REC, arg, ex);
  if (i >= n || !real_lane()) return;
  const u32 k = my_pair();
  // the line functions report Fq2 number k as it is; an element's flat coefficient k goes back to its place in the tower's memory order
  const u32 pos = (OP == KEAKI_TOP_W_LINE_DOUBLE || OP == KEAKI_TOP_W_LINE_ADD) ? k : (k & 1u) * 3u + (k >> 1);
  st_fq(out + (size_t)i * OUT, 2u * pos + lane_odd(), r);
}
template <int OP>
void launch(hipStream_t s, const u32* in, u32 n, u32 blocks, u32* out, int arg) {
  hipLaunchKernelGGL((k_tower_probe_wide<OP>), dim3(blocks), dim3(64), 0, s, in, n, out, arg);
}
#define E(op) {&launch<KEAKI_TOP_##op>, 0}
static const Entry TABLE[KEAKI_TOP_COUNT - KEAKI_TOP_FIRST_WIDE] = {
  E(W12_MUL), E(W12_MUL_034), E(W12_CYC_SQR), {&launch<KEAKI_TOP_W12_FROB1>, 1}, {&launch<KEAKI_TOP_W12_FROB1>, 2}, {&launch<KEAKI_TOP_W12_FROB1>, 3},
  E(W12_CONJ), E(W12_INV), E(W12_GATHER_OWN), E(W_LINE_DOUBLE), E(W_LINE_ADD),
};
#undef E
static_assert(KEAKI_TOP_W12_MUL == KEAKI_TOP_FIRST_WIDE && KEAKI_TOP_W12_FROB1 == KEAKI_TOP_FIRST_WIDE + 3 && KEAKI_TOP_W12_CONJ == KEAKI_TOP_FIRST_WIDE + 6 &&
              KEAKI_TOP_W_LINE_ADD == KEAKI_TOP_FIRST_WIDE + 10 && KEAKI_TOP_COUNT == KEAKI_TOP_FIRST_WIDE + 11, "tower probe: the table follows the enum");
}  // namespace tprobe
}  // namespace bn254

namespace keaki_internal {
void tower_probe_wide_launch(hipStream_t s, uint32_t wide_op, const uint32_t* in, uint32_t n, uint32_t blocks, uint32_t* out) {
  const bn254::tprobe::Entry& e = bn254::tprobe::TABLE[wide_op];
  e.launch(s, in, n, blocks, out, e.arg);
}
}  // namespace keaki_internal
