// Square-root exponentiation in Fq: a^((p+1)/4), the root candidate for p = 3 (mod 4) (point_codec.hip; the caller squares it to check).
// A fixed sliding window over the constant exponent: odd powers a, a^3, a^5, a^7, windows of at most three bits -- 251 squarings and 58
// products (three of them, and one squaring, for the odd powers; the first window only loads its power) where bit-by-bit square-and-multiply takes 252 + 109. Every decision depends on the exponent only, so the whole wave walks one path and
// the schedule lives in scalar registers.
// Written once over the field form (bench_tools/ubench_sqrt_forms.hip times the two on one device; the library instantiates PowU29):
//   PowU29   nine 29-bit lazy limbs, radix 2^261 (fq29_core.hip.h): a square is 45 + 81 multiply-adds and no carry chain
//   PowSat   eight saturated 32-bit limbs, radix 2^256 (bn254_field_asm.hip.h): the product stream serves as the square
#pragma once
#include "bn254_field.hip.h"

namespace bn254 {

// (p + 1) / 4, little-endian words, 252 bits (tests/test_point_codec_model.py checks the words against the big-int value)
__device__ __constant__ const uint32_t FQ_SQRT_EXP[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
constexpr int FQ_SQRT_EXP_BITS = 252;

struct PowU29 {
  using T = U29;
  static KDEV T load(const Fq& a) { return u29_mul(u29_from_sat_shift5(a.l), u29_const(Fq29Params::ONE)); }   // 2^261 form, below 2p
  static KDEV T mul(const T& a, const T& b) { return u29_mul(a, b); }
  static KDEV T sqr(const T& a) { return u29_sqr(a); }
  static KDEV Fq store(const T& a) { Fq r; u29_pack_canonical(r.l, u29_mul(a, u29_const(Fq29Params::R256))); return r; }
};
struct PowSat {
  using T = Fq;
  static KDEV T load(const Fq& a) { return a; }
  static KDEV T mul(const T& a, const T& b) { return a * b; }
  static KDEV T sqr(const T& a) { return a * a; }
  static KDEV Fq store(const T& a) { return a; }
};

KDEV u32 fq_sqrt_exp_bit(int i) { return (FQ_SQRT_EXP[i >> 5] >> (i & 31)) & 1u; }

// a^((p+1)/4) for a Montgomery residue a (2^256 form, canonical); the result in the same form
template <class F>
KDEV Fq fq_pow_sqrt_exp(const Fq a) {
  using T = typename F::T;
  const T b1 = F::load(a);
  const T b2 = F::sqr(b1);
  const T b3 = F::mul(b1, b2), b5 = F::mul(b3, b2), b7 = F::mul(b5, b2);
  T acc = b1;                                    // overwritten by the first window (the top bit of the exponent is set): no squarings of one
  bool started = false;
  int i = FQ_SQRT_EXP_BITS - 1;
#pragma unroll 1
  while (i >= 0) {
    int len = 1;
    u32 win = 0;
    if (fq_sqrt_exp_bit(i)) {                    // the longest window of at most three bits that ends in a one
      len = i >= 2 ? 3 : i + 1;
      while (!fq_sqrt_exp_bit(i - len + 1)) len--;
#pragma unroll 1
      for (int k = 0; k < len; k++) win = (win << 1) | fq_sqrt_exp_bit(i - k);
    }
#pragma unroll 1
    for (int k = 0; started && k < len; k++) acc = F::sqr(acc);
    if (win) {
      T m;
#pragma unroll
      for (int j = 0; j < (int)(sizeof(T) / sizeof(u32)); j++) m.l[j] = win == 1 ? b1.l[j] : win == 3 ? b3.l[j] : win == 5 ? b5.l[j] : b7.l[j];
      acc = started ? F::mul(acc, m) : m;
      started = true;
    }
    i -= len;
  }
  return F::store(acc);
}

}  // namespace bn254
