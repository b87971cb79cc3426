// Fr helpers shared by the KZG kernels (kzg_batch.hip, kzg_each.hip, kzg_cosets.hip, kzg_multi.hip, vec_update.hip).
#pragma once
#include "bn254_field.hip.h"

namespace bn254 {

// base^e by square-and-multiply from the low bit (e < 2^32: at most 32 squarings): omega^i of the calls that take a domain generator
KDEV Fr fr_pow_u32(Fr base, u32 e) {
  Fr acc = fp_one<FrParams>();
#pragma unroll 1
  while (e) {
    if (e & 1u) acc = fp_mul<FrParams>(acc, base);
    base = fp_mul<FrParams>(base, base);
    e >>= 1;
  }
  return acc;
}

// x^(r - 2) (Fermat), 0 -> 0: the ONE Fr inversion of the library (set_polys' weights, vec_update's table, the shifts of verify_cosets)
KDEV Fr fr_inv(const Fr& x) {
  Fr acc = fp_one<FrParams>();
#pragma unroll 1
  for (int wi = 7; wi >= 0; wi--) {
    const u32 word = wi ? FrParams::MOD[wi] : FrParams::MOD[0] - 2u;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = fp_mul<FrParams>(acc, acc);
      if ((word >> b) & 1u) acc = fp_mul<FrParams>(acc, x);
    }
  }
  return acc;
}

// sum over the 64 lanes of a wave by cross-lane moves; every lane ends up with the total
KDEV Fr fr_wave_sum(Fr a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Fr o;
#pragma unroll
    for (int j = 0; j < 8; j++) o.l[j] = (u32)__shfl_xor((int)a.l[j], off, 64);
    a = fp_add<FrParams>(a, o);
  }
  return a;
}

}  // namespace bn254
