// Point probe, shared by its two translation units (point_probe.hip: G1, GLV, ladders and the saturated formulas over Fq; point_probe_g2.hip:
// xyzz29_g2.hip.h and the saturated formulas over Fq2): the record's geometry (include/keaki_hip.h), the loads and stores of one lane, the
// kernel frame and the saturated ops written once for both fields. No arithmetic here.
#pragma once
#include "bn254_curve.hip.h"
#include "fq29.hip.h"
#include "internal.h"

namespace bn254 {
namespace pprobe {
constexpr int SW = KEAKI_POP_SLOT_WORDS, REC = KEAKI_POP_SLOTS * SW, OUT = KEAKI_POP_OUT_SLOTS * SW;
constexpr int FLAGS = KEAKI_POP_FLAG_SLOT * SW, OFLAGS = KEAKI_POP_OUT_FLAG_SLOT * SW;

KDEV U29 ld_u(const u32* rec, int s) {
  U29 r;
#pragma unroll
  for (int j = 0; j < 9; j++) r.l[j] = rec[s * SW + j];
  return r;
}
template <class F>
KDEV F ld_w(const u32* rec, int s) {      // eight words: Fq or Fr
  F r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = rec[s * SW + j];
  return r;
}
KDEV void st_u(u32* out, int s, const U29& x) {
#pragma unroll
  for (int j = 0; j < 9; j++) out[s * SW + j] = x.l[j];
}
KDEV void st_q(u32* out, int s, const Fq& x) {
#pragma unroll
  for (int j = 0; j < 8; j++) out[s * SW + j] = x.l[j];
}
// a saturated coordinate at slot s: one slot over Fq, two (c0, c1) over Fq2
template <class F> KDEV F ld_f(const u32* rec, int s);
template <> KDEV Fq ld_f<Fq>(const u32* rec, int s) { return ld_w<Fq>(rec, s); }
template <> KDEV Fq2 ld_f<Fq2>(const u32* rec, int s) { return {ld_w<Fq>(rec, s), ld_w<Fq>(rec, s + 1)}; }
KDEV void st_f(u32* out, int s, const Fq& x) { st_q(out, s, x); }
KDEV void st_f(u32* out, int s, const Fq2& x) { st_q(out, s, x.c0); st_q(out, s + 1, x.c1); }
template <class F> constexpr int fslots() { return sizeof(F) / sizeof(Fq); }

template <class F> KDEV Aff<F> ld_aff(const u32* rec, int s) { return {ld_f<F>(rec, s), ld_f<F>(rec, s + fslots<F>())}; }
template <class F> KDEV Jac<F> ld_jac(const u32* rec, int s) { return {ld_f<F>(rec, s), ld_f<F>(rec, s + fslots<F>()), ld_f<F>(rec, s + 2 * fslots<F>())}; }
template <class F> KDEV Xyzz<F> ld_xyzz(const u32* rec, int s) {
  return {ld_f<F>(rec, s), ld_f<F>(rec, s + fslots<F>()), ld_f<F>(rec, s + 2 * fslots<F>()), ld_f<F>(rec, s + 3 * fslots<F>())};
}
template <class F> KDEV void st_jac(u32* out, const Jac<F>& p) { st_f(out, 0, p.x); st_f(out, fslots<F>(), p.y); st_f(out, 2 * fslots<F>(), p.z); }
template <class F> KDEV void st_xyzz(u32* out, const Xyzz<F>& p) {
  st_f(out, 0, p.x); st_f(out, fslots<F>(), p.y); st_f(out, 2 * fslots<F>(), p.zz); st_f(out, 3 * fslots<F>(), p.zzz);
}

// the saturated formulas: `which` counts from the field's XYZZ_ADD_MIXED op
template <class F, int WHICH>
KDEV void run_sat(const u32* rec, u32* o) {
  constexpr int S = fslots<F>();
  if constexpr (WHICH == 0) st_xyzz(o, xyzz_add_mixed(ld_xyzz<F>(rec, 0), ld_aff<F>(rec, 4 * S)));
  else if constexpr (WHICH == 1) st_xyzz(o, xyzz_add(ld_xyzz<F>(rec, 0), ld_xyzz<F>(rec, 4 * S)));
  else if constexpr (WHICH == 2) st_xyzz(o, xyzz_dbl(ld_xyzz<F>(rec, 0)));
  else if constexpr (WHICH == 3) st_xyzz(o, xyzz_dbl_aff(ld_aff<F>(rec, 0)));
  else if constexpr (WHICH == 4) st_jac(o, jac_add(ld_jac<F>(rec, 0), ld_jac<F>(rec, 3 * S)));
  else if constexpr (WHICH == 5) st_jac(o, jac_add_mixed(ld_jac<F>(rec, 0), ld_aff<F>(rec, 3 * S)));
  else if constexpr (WHICH == 6) st_jac(o, jac_dbl(ld_jac<F>(rec, 0)));
  else static_assert(WHICH < 0, "point probe: saturated op without a body");
}

typedef void (*Launch)(hipStream_t, const u32*, u32, u32, u32*, uint4*);
}  // namespace pprobe
}  // namespace bn254

namespace keaki_internal {
// op - KEAKI_POP_FIRST_G2 of the ops of point_probe_g2.hip
void point_probe_g2_launch(hipStream_t s, uint32_t g2_op, const uint32_t* in, uint32_t n, uint32_t blocks, uint32_t* out);
}  // namespace keaki_internal
