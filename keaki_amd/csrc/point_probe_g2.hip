// Point probe (keaki_hip_selftest_point_ops), G2 half: the lazy-limb XYZZ arithmetic over Fq2 (xyzz29_g2.hip.h: the G2 bucket kernel, the G2
// tail, the ciphertext side of `encapsulate`) and the saturated formulas over Fq2 that the G2 ladders run (bn254_curve.hip.h), ONE call per
// kernel on operands chosen by the host. Frame, record layout and what is not probed: point_probe.hip, include/keaki_hip.h.
#define KEAKI_FQ2_OUTLINE 1
#include <array>

#include "point_probe.hip.h"
#include "xyzz29_g2.hip.h"
namespace bn254 {
namespace pprobe {
constexpr int G2 = KEAKI_POP_FIRST_G2;
KDEV L2 ld_l2(const u32* rec, int s) { return {ld_u(rec, s), ld_u(rec, s + 1)}; }
KDEV X29G2 ld_x29g2(const u32* rec, int s, int flag) { return {ld_l2(rec, s), ld_l2(rec, s + 2), ld_l2(rec, s + 4), ld_l2(rec, s + 6), rec[FLAGS + flag] != 0}; }
KDEV void st_x29g2(u32* o, const X29G2& p) {
  st_u(o, 0, p.x.a); st_u(o, 1, p.x.b); st_u(o, 2, p.y.a); st_u(o, 3, p.y.b);
  st_u(o, 4, p.zz.a); st_u(o, 5, p.zz.b); st_u(o, 6, p.zzz.a); st_u(o, 7, p.zzz.b);
  o[OFLAGS] = p.empty ? 1u : 0u;
}

template <int OP>
KDEV void run_g2(const u32* rec, u32* o) {
  if constexpr (OP == KEAKI_POP_X29G2_ADD_MIXED) {
    X29G2 acc = ld_x29g2(rec, 0, 0);
    x29g2_add_mixed(acc, ld_aff<Fq2>(rec, 8));
    st_x29g2(o, acc);
  } else if constexpr (OP == KEAKI_POP_X29G2_ADD) st_x29g2(o, x29g2_add(ld_x29g2(rec, 0, 0), ld_x29g2(rec, 8, 1)));
  else if constexpr (OP == KEAKI_POP_X29G2_DBL) st_x29g2(o, x29g2_dbl(ld_x29g2(rec, 0, 0)));
  else if constexpr (OP == KEAKI_POP_X29G2_DBL_OF_ACC) st_x29g2(o, x29g2_dbl_of_acc(ld_x29g2(rec, 0, 0)));
  else if constexpr (OP == KEAKI_POP_X29G2_STORE) st_xyzz(o, x29g2_store(ld_x29g2(rec, 0, 0)));
  else if constexpr (OP >= KEAKI_POP_XYZZ_ADD_MIXED_FQ2 && OP <= KEAKI_POP_JAC_DBL_FQ2) run_sat<Fq2, OP - KEAKI_POP_XYZZ_ADD_MIXED_FQ2>(rec, o);
  else static_assert(OP < 0, "point probe: G2 op without a body");
}

template <int OP>
__global__ void __launch_bounds__(64) k_point_probe_g2(const u32* __restrict__ in, u32* __restrict__ out) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  run_g2<OP>(in + (size_t)i * REC, out + (size_t)i * OUT);
}
template <int OP>
void launch_g2(hipStream_t s, const u32* in, u32 n, u32 blocks, u32* out, uint4*) {
  hipLaunchKernelGGL((k_point_probe_g2<OP>), dim3(blocks), dim3(64), 0, s, in, out);
}
template <int... OPS>
constexpr std::array<Launch, sizeof...(OPS)> make_table(std::integer_sequence<int, OPS...>) { return {{&launch_g2<G2 + OPS>...}}; }
static const auto TABLE = make_table(std::make_integer_sequence<int, KEAKI_POP_COUNT - G2>{});
}  // namespace pprobe
}  // namespace bn254

namespace keaki_internal {
void point_probe_g2_launch(hipStream_t s, uint32_t g2_op, const uint32_t* in, uint32_t n, uint32_t blocks, uint32_t* out) {
  bn254::pprobe::TABLE[g2_op](s, in, n, blocks, out, nullptr);
}
}  // namespace keaki_internal
