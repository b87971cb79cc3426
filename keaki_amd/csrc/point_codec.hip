// Compressed point wire format (keaki_hip_g1/g2_compress, _decompress, keaki_hip_g2_subgroup_check): ark-serialize 0.4.2
// `serialize_compressed` of short-Weierstrass affine points -- x as canonical little-endian integers (G1 32 B; G2 x.c0 then x.c1, 64 B), bit 7
// of the last byte set iff y > -y (Fq: canonical integers; Fq2: c1 decides, c0 when c1 = 0), bit 6 = identity with x = 0. One lane per point.
//   k_compress<F>        leaves Montgomery form, compares y with (p - 1)/2, writes the bytes
//   k_decompress<F>      flags and x < p (status 1), y = sqrt(x^3 + b) checked by squaring (status 2), the root the flag names; a rejected item
//                        decodes to all-zero words
//   k_g2_subgroup        psi(Q) == [6 z^2]Q (status 3): Jacobian double-and-add over the 127-bit constant, compared without an inversion
// Square roots: Fq by a^((p+1)/4) (fq_sqrt.hip.h); Fq2 by the complex method with ONE inversion: alpha = sqrt(a0^2 + a1^2), delta = (a0 + alpha)/2,
// x = delta^((p+1)/4); x^2 = delta gives (x, a1/(2x)), otherwise x^2 = -delta, the other delta' = (a0 - alpha)/2 = -a1^2/(4 delta) has the root
// a1/(2x) and the result is (a1/(2x), x). Two exponentiations and one division-step inverse per G2 point; a final squaring decides.
// The model of all of it: tests/point_codec_model.py.
#include "internal.h"
#include "bn254_curve.hip.h"
#include "fq_sqrt.hip.h"

namespace bn254 {

constexpr u32 PC_THREADS = 64;
// (p - 1) / 2: y > -y  <=>  y > (p - 1) / 2 on canonical integers
__device__ __constant__ const uint32_t FQ_HALF[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
// 6 z^2 (127 bits): psi acts on G2 as multiplication by p, and p = 6 z^2 (mod r)
constexpr u64 SIX_Z2_LO = 0xf83e9682e87cfd46ull, SIX_Z2_HI = 0x6f4d8248eeb859fbull;
constexpr int SIX_Z2_BITS = 127;
static_assert((unsigned __int128)BN_Z * BN_Z * 6 == (((unsigned __int128)SIX_Z2_HI << 64) | SIX_Z2_LO), "6 z^2");

static __device__ __noinline__ Fq fq_pow_sqrt(const Fq a) { return fq_pow_sqrt_exp<PowU29>(a); }
// a^-1 through the division steps, operand by value (fq_inv takes a reference, which would send the caller's copy through scratch memory): the
// integer a R has the inverse a^-1 R^-1, one product by R^3 brings the Montgomery form back; 0 -> 0
KDEV Fq fq_inv_by_value(const Fq a) {
  Fq r3;
#pragma unroll
  for (int i = 0; i < 8; i++) r3.l[i] = FqParams::R3[i];
  return fq_inv_safegcd_words(a) * r3;
}

// canonical words w > (p - 1) / 2
KDEV bool words_gt_half(const u32* w) {
  u32 borrow = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 d = (u64)FQ_HALF[j] - w[j] - borrow;
    borrow = (u32)(d >> 63);
  }
  return borrow != 0;
}
// canonical words w >= p
KDEV bool words_ge_p(const u32* w) {
  u32 borrow = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 d = (u64)w[j] - FqParams::MOD[j] - borrow;
    borrow = (u32)(d >> 63);
  }
  return borrow == 0;
}
KDEV bool words_zero(const u32* w) {
  u32 o = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) o |= w[j];
  return o == 0;
}

// the YIsNegative flag, from Montgomery residues
KDEV bool y_is_neg(const Fq& y) {
  u32 w[8];
  fp_from_mont<FqParams>(w, y);
  return words_gt_half(w);
}
KDEV bool y_is_neg(const Fq2& y) {
  u32 w0[8], w1[8];
  fp_from_mont<FqParams>(w0, y.c0);
  fp_from_mont<FqParams>(w1, y.c1);
  return words_zero(w1) ? words_gt_half(w0) : words_gt_half(w1);
}

// a root of a, or ok = false
KDEV Fq f_sqrt(const Fq& a, bool& ok) {
  const Fq c = fq_pow_sqrt(a);
  ok = fq_eq(fq_sqr(c), a);
  return c;
}
KDEV Fq2 f_sqrt(const Fq2& a, bool& ok) {
  Fq2 c;
  if (fq_is_zero(a.c1)) {                    // a in Fq: (sqrt(a0), 0), or (0, sqrt(-a0)) for a non-residue a0
    const Fq x = fq_pow_sqrt(a.c0);
    const bool res = fq_eq(fq_sqr(x), a.c0);
    c.c0 = res ? x : fq_zero();
    c.c1 = res ? fq_zero() : x;
  } else {
    const Fq alpha = fq_pow_sqrt(fq_sqr(a.c0) + fq_sqr(a.c1));
    const Fq delta = (a.c0 + alpha) * FQ_TWO_INV;
    const Fq x = fq_pow_sqrt(delta);
    const Fq t = a.c1 * fq_inv_by_value(fq_dbl(x));
    const bool res = fq_eq(fq_sqr(x), delta);
    c.c0 = res ? x : t;
    c.c1 = res ? t : x;
  }
  ok = fq2_eq(fq2_sqr(c), a);                 // also what rejects a non-square: alpha was no root of the norm then
  return c;
}

KDEV Fq curve_b_of(const Fq*) {
  const Fq one = fq_one();
  return one + one + one;
}
KDEV Fq2 curve_b_of(const Fq2*) { return G2_B; }

template <class F> struct Coords;
template <> struct Coords<Fq> {
  static constexpr int N = 1;
  static KDEV const Fq& get(const Fq& x, int) { return x; }
  static KDEV void set(Fq& x, int, const Fq& v) { x = v; }
};
template <> struct Coords<Fq2> {
  static constexpr int N = 2;
  static KDEV const Fq& get(const Fq2& x, int k) { return k ? x.c1 : x.c0; }
  static KDEV void set(Fq2& x, int k, const Fq& v) { if (k) x.c1 = v; else x.c0 = v; }
};

// ---- compress: n affine points (Montgomery limbs, (0, 0) = identity) -> n x 32 B / 64 B ---------------------------------------------------------
template <class F>
static __global__ void __launch_bounds__(256) k_compress(const Aff<F>* __restrict__ pts, u32 n, uint4* __restrict__ out) {
  constexpr int NC = Coords<F>::N;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Aff<F> p = pts[i];
  u32 w[8 * NC];
  if (aff_is_inf(p)) {
#pragma unroll
    for (int j = 0; j < 8 * NC; j++) w[j] = 0;
    w[8 * NC - 1] = 0x40000000u;
  } else {
#pragma unroll
    for (int k = 0; k < NC; k++) fp_from_mont<FqParams>(w + 8 * k, Coords<F>::get(p.x, k));
    if (y_is_neg(p.y)) w[8 * NC - 1] |= 0x80000000u;
  }
#pragma unroll
  for (int j = 0; j < 2 * NC; j++) out[(size_t)i * (2 * NC) + j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

// ---- decompress ---------------------------------------------------------------------------------------------------------------------------------
// status (optional): 0 ok, 1 malformed, 2 not on the curve. bad2 = {count, first index} over base + i (the host form runs in chunks).
template <class F>
static __global__ void __launch_bounds__(PC_THREADS) k_decompress(const uint4* __restrict__ in, u32 n, unsigned long long base, Aff<F>* __restrict__ out,
                                                                  uint8_t* __restrict__ status, unsigned long long* __restrict__ bad2) {
  constexpr int NC = Coords<F>::N;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 w[8 * NC];
#pragma unroll
  for (int j = 0; j < 2 * NC; j++) {
    const uint4 v = in[(size_t)i * (2 * NC) + j];
    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
  }
  const bool neg = (w[8 * NC - 1] >> 31) != 0, inf = ((w[8 * NC - 1] >> 30) & 1u) != 0;
  w[8 * NC - 1] &= 0x3fffffffu;
  bool range_ok = true, x_zero = true;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    range_ok = range_ok && !words_ge_p(w + 8 * k);
    x_zero = x_zero && words_zero(w + 8 * k);
  }
  u32 st = 0;
  Aff<F> p = aff_inf<F>();
  if ((neg && inf) || !range_ok || (inf && !x_zero)) {
    st = 1;
  } else if (!inf) {
    F x;
#pragma unroll
    for (int k = 0; k < NC; k++) Coords<F>::set(x, k, fp_to_mont<FqParams>(w + 8 * k));
    bool ok;
    const F y = f_sqrt(f_sqr(x) * x + curve_b_of((const F*)nullptr), ok);
    if (ok) {
      p.x = x;
      p.y = f_cneg(y, y_is_neg(y) != neg);
    } else {
      st = 2;
    }
  }
  out[i] = p;
  if (status) status[i] = (uint8_t)st;
  if (st) {
    atomicAdd(bad2, 1ull);
    atomicMin(bad2 + 1, base + i);
  }
}

// ---- G2 subgroup test ---------------------------------------------------------------------------------------------------------------------------
// psi(x, y) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)); on G2 it is multiplication by p = 6 z^2 (mod r), and no other point of the twist satisfies
// psi(Q) = [6 z^2]Q (tests/test_point_codec_model.py: against [r]Q = O). The accumulator [k]Q stays Jacobian and is compared with the affine
// psi(Q) through its own Z: X == x Z^2, Y == y Z^3. The additions branch on equal and opposite operands and on an identity accumulator: inside G2
// none of them occurs (k < r), points of the twist outside G2 (the cofactor 2p - r has the factor 10069) can meet all three.
// The ladder's field: Fq2 whose products are real functions (one copy of each stream: the loop stays inside the instruction cache). A function has
// 31 argument registers and the two operands of an Fq2 product are 32 words (4 x 254 bits do not fit 31 words either). Two forms, measured
// against each other on one device (profiles/point_codec.txt):
//   shipped                   ONE out-of-line Fq2 product, the dual product of fq29_core.hip.h (~770 instructions), operands as two 16-word vectors:
//                             31 words in registers, the 32nd over the stack -- 8 bytes of private segment per lane, one scratch store and load of a
//                             single word per product, no spill. 2^20 subgroup tests in 41.5 ms.
//   -DKEAKI_CODEC_FQ_CALLS    the out-of-line unit is the Fq product (two 8-word vectors in, one out: everything in registers, no private segment,
//                             no scratch instruction); an Fq2 product is three of them (Karatsuba, ~1,050 instructions), a square two. 51.7 ms.
// The register-only form is 25 % slower, so the form with the one stack word ships. The curve formulas of bn254_curve.hip.h are instantiated over
// either unchanged.
#ifdef KEAKI_CODEC_FQ_CALLS
typedef u32 u32x8 __attribute__((ext_vector_type(8)));
KDEV u32x8 fq_pack(const Fq& a) {
  u32x8 v;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = a.l[j];
  return v;
}
KDEV Fq fq_unpack(const u32x8 v) {
  Fq a;
#pragma unroll
  for (int j = 0; j < 8; j++) a.l[j] = v[j];
  return a;
}
static __device__ __noinline__ u32x8 fq_mul_vec(const u32x8 a, const u32x8 b) { return fq_pack(fq_unpack(a) * fq_unpack(b)); }
KDEV Fq fq_mul_call(const Fq& a, const Fq& b) { return fq_unpack(fq_mul_vec(fq_pack(a), fq_pack(b))); }
KDEV Fq2 fq2_mul_call(const Fq2& a, const Fq2& b) {      // (a0 b0 - a1 b1) + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
  const Fq v0 = fq_mul_call(a.c0, b.c0), v1 = fq_mul_call(a.c1, b.c1);
  return {v0 - v1, fq_mul_call(a.c0 + a.c1, b.c0 + b.c1) - v0 - v1};
}
KDEV Fq2 fq2_sqr_call(const Fq2& a) {                    // (a0 + a1)(a0 - a1) + 2 a0 a1 u
  return {fq_mul_call(a.c0 + a.c1, a.c0 - a.c1), fq_dbl(fq_mul_call(a.c0, a.c1))};
}
#else
typedef u32 u32x16 __attribute__((ext_vector_type(16)));
KDEV u32x16 fq2_pack(const Fq2& a) {
  u32x16 v;
#pragma unroll
  for (int j = 0; j < 8; j++) { v[j] = a.c0.l[j]; v[8 + j] = a.c1.l[j]; }
  return v;
}
KDEV Fq2 fq2_unpack(const u32x16 v) {
  Fq2 a;
#pragma unroll
  for (int j = 0; j < 8; j++) { a.c0.l[j] = v[j]; a.c1.l[j] = v[8 + j]; }
  return a;
}
static __device__ __noinline__ u32x16 fq2_mul_vec(const u32x16 a, const u32x16 b) { return fq2_pack(fq2_mul_inl(fq2_unpack(a), fq2_unpack(b))); }
static __device__ __noinline__ u32x16 fq2_sqr_vec(const u32x16 a) { return fq2_pack(fq2_sqr_inl(fq2_unpack(a))); }
KDEV Fq2 fq2_mul_call(const Fq2& a, const Fq2& b) { return fq2_unpack(fq2_mul_vec(fq2_pack(a), fq2_pack(b))); }
KDEV Fq2 fq2_sqr_call(const Fq2& a) { return fq2_unpack(fq2_sqr_vec(fq2_pack(a))); }
#endif
struct Fq2L {
  Fq2 v;
};
KDEV Fq2L operator+(const Fq2L& a, const Fq2L& b) { return {a.v + b.v}; }
KDEV Fq2L operator-(const Fq2L& a, const Fq2L& b) { return {a.v - b.v}; }
KDEV Fq2L operator-(const Fq2L& a) { return {-a.v}; }
KDEV Fq2L operator*(const Fq2L& a, const Fq2L& b) { return {fq2_mul_call(a.v, b.v)}; }
KDEV Fq2L f_sqr(const Fq2L& a) { return {fq2_sqr_call(a.v)}; }
KDEV Fq2L f_dbl(const Fq2L& a) { return {fq2_dbl(a.v)}; }
KDEV bool f_is_zero(const Fq2L& a) { return fq2_is_zero(a.v); }
KDEV bool f_eq(const Fq2L& a, const Fq2L& b) { return fq2_eq(a.v, b.v); }
template <> KDEV Fq2L f_zero<Fq2L>() { return {fq2_zero()}; }
template <> KDEV Fq2L f_one<Fq2L>() { return {fq2_one()}; }

KDEV bool g2_in_subgroup(const G2Aff& q) {
  if (aff_is_inf(q)) return true;
  const Aff<Fq2L> ql = {{q.x}, {q.y}};
  Jac<Fq2L> acc = {ql.x, ql.y, f_one<Fq2L>()};
#pragma unroll 1
  for (int i = SIX_Z2_BITS - 2; i >= 0; i--) {
    acc = jac_dbl(acc);
    if (((i < 64 ? SIX_Z2_LO : SIX_Z2_HI) >> (i & 63)) & 1ull) acc = jac_add_mixed(acc, ql);
  }
  if (jac_is_inf(acc)) return false;           // psi(Q) is a point of the curve, never the identity
  const Fq2L px = Fq2L{fq2_conj(q.x)} * Fq2L{TWIST_MUL_BY_Q_X}, py = Fq2L{fq2_conj(q.y)} * Fq2L{TWIST_MUL_BY_Q_Y};
  const Fq2L zz = f_sqr(acc.z);
  return f_eq(acc.x, px * zz) && f_eq(acc.y, py * zz * acc.z);
}

// pts: n affine points. An outsider counts into bad2 (as in k_decompress); with `status` it gets 3 there, with `clear` its point becomes all-zero
// words (the decompress path, where rejected items -- already zero, hence members -- must stay rejected).
static __global__ void __launch_bounds__(PC_THREADS) k_g2_subgroup(G2Aff* __restrict__ pts, u32 n, unsigned long long base, uint8_t* __restrict__ status,
                                                                   int clear, unsigned long long* __restrict__ bad2) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G2Aff q = pts[i];
  if (g2_in_subgroup(q)) return;
  if (status) status[i] = 3;
  if (clear) pts[i] = aff_inf<Fq2>();
  atomicAdd(bad2, 1ull);
  atomicMin(bad2 + 1, base + i);
}

}  // namespace bn254

namespace keaki_internal {
using namespace bn254;

keaki_status point_compress_run(keaki_hip_ctx* ctx, bool g2, const void* d_pts, size_t n, void* d_out) {
  if (n == 0) return KEAKI_OK;
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "point codec: n must be < 2^31 per call");
  if (g2) hipLaunchKernelGGL((k_compress<Fq2>), dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const G2Aff*)d_pts, (u32)n, (uint4*)d_out);
  else hipLaunchKernelGGL((k_compress<Fq>), dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const G1Aff*)d_pts, (u32)n, (uint4*)d_out);
  return launch_check(ctx, "point_compress");
}

keaki_status point_decompress_run(keaki_hip_ctx* ctx, bool g2, const void* d_bytes, size_t n, uint64_t base, void* d_out, void* d_status, void* d_bad2) {
  if (n == 0) return KEAKI_OK;
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "point codec: n must be < 2^31 per call");
  if (g2)
    hipLaunchKernelGGL((k_decompress<Fq2>), dim3(cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, ctx->stream, (const uint4*)d_bytes, (u32)n,
                       (unsigned long long)base, (G2Aff*)d_out, (uint8_t*)d_status, (unsigned long long*)d_bad2);
  else
    hipLaunchKernelGGL((k_decompress<Fq>), dim3(cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, ctx->stream, (const uint4*)d_bytes, (u32)n,
                       (unsigned long long)base, (G1Aff*)d_out, (uint8_t*)d_status, (unsigned long long*)d_bad2);
  return launch_check(ctx, "point_decompress");
}

keaki_status g2_subgroup_run(keaki_hip_ctx* ctx, void* d_pts, size_t n, uint64_t base, void* d_status, bool clear, void* d_bad2) {
  if (n == 0) return KEAKI_OK;
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "point codec: n must be < 2^31 per call");
  hipLaunchKernelGGL(k_g2_subgroup, dim3(cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, ctx->stream, (G2Aff*)d_pts, (u32)n, (unsigned long long)base,
                     (uint8_t*)d_status, clear ? 1 : 0, (unsigned long long*)d_bad2);
  return launch_check(ctx, "g2_subgroup");
}

}  // namespace keaki_internal
