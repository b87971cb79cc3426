// Fr helpers shared by the KZG verification kernels (kzg_batch.hip, kzg_each.hip).
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

}  // namespace bn254
