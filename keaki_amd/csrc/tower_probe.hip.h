// Tower probe, shared by its two translation units (tower_probe.hip: the lane-pair form, tower_probe_wide.hip: the twelve-lane form): the
// record's areas (include/keaki_hip.h) and the loads and stores of one lane. No arithmetic here.
#pragma once
#include "pairing_wide.hip.h"
#include "internal.h"

namespace bn254 {
namespace tprobe {
constexpr int REC = KEAKI_TOP_REC_WORDS, OUT = KEAKI_TOP_OUT_WORDS;
constexpr int A_OFF = 0, B_OFF = 96, LINE_OFF = 192, T_OFF = 246, Q_OFF = 294, P_OFF = 326;
static_assert(P_OFF + 18 == REC && OUT == 96, "tower probe: record layout");

// Fq number i (8 words) of the area at `off`
KDEV Fq ld_fq(const u32* rec, int off, u32 i) {
  Fq r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = rec[off + 8u * i + j];
  return r;
}
// limb vector number i (9 limbs) of the area at `off`
KDEV U29 ld_limbs(const u32* rec, int off, u32 i) {
  U29 r;
#pragma unroll
  for (int j = 0; j < 9; j++) r.l[j] = rec[off + 9u * i + j];
  return r;
}
KDEV void st_fq(u32* out, u32 i, const Fq& v) {
#pragma unroll
  for (int j = 0; j < 8; j++) out[8u * i + j] = v.l[j];
}

typedef void (*Launch)(hipStream_t, const u32*, u32, u32, u32*, int);
struct Entry { Launch launch; int arg; };
}  // namespace tprobe
}  // namespace bn254

namespace keaki_internal {
// op - KEAKI_TOP_FIRST_WIDE of the wide ops (tower_probe_wide.hip)
void tower_probe_wide_launch(hipStream_t s, uint32_t wide_op, const uint32_t* in, uint32_t n, uint32_t blocks, uint32_t* out);
}  // namespace keaki_internal
