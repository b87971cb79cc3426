// KZG verify_each, pairing side: valid_i <=> e(L_i, g2) * e(-proof_i, [tau]_2) == 1 with BOTH second arguments fixed for the call, so both line
// sequences are tables (k_g2_prepare). One lane pair per item, as k_pairing (pairing.hip.h), whose device functions run here as they are: the
// loop over MILLER_STEPS squares f once per step and multiplies it by the line of table A at L_i and by the line of table B at -proof_i -- 64
// squarings for the two pairings together -- then ONE final exponentiation (fe_run) and a comparison with one: a byte out, not 384.
// With both slots on tabulated lines no running point T is held, so park indices 0..1 carry the second point; PARK_CHUNKS and the LDS footprint
// are k_pairing's. A translation unit of its own: k_pairing's generated code does not depend on this kernel in any way.
#define KEAKI_FQ2_OUTLINE 1
#include "internal.h"
#include "pairing.hip.h"
namespace keaki_internal {
using namespace bn254;

// f = prod over the steps of (f^2 if the step squares) * l_A(P1) * l_B(P2). Parked: P1 in 6..7, P2 in 0..1; the squaring and the line product
// use 3..5 for their temporaries.
static KTOWER void miller_loop2(Fq12* f, const Fq& p1x, const Fq& p1y, const Fq& p2x, const Fq& p2y, const Line* __restrict__ lines_a,
                                const Line* __restrict__ lines_b, uint4* park) {
  const u32 par = lane_odd();
  fq12_set_one(f);
  park_fq(park, 6, p1x); park_fq(park, 7, p1y);
  park_fq(park, 0, p2x); park_fq(park, 1, p2y);
#pragma unroll 1
  for (int li = 0; li < MILLER_NSTEPS; li++) {
    if (MILLER_STEPS[li] == 1) fq12_sqr<true>(f, f, park, 3);
    Line l = lines_a[li * 2 + par];
    ell(f, &l, cut(unpark_fq(park, 6)), cut(unpark_fq(park, 7)), park, 3);
    l = lines_b[li * 2 + par];
    ell(f, &l, cut(unpark_fq(park, 0)), cut(unpark_fq(park, 1)), park, 3);
  }
}

struct Pair2Args {
  const G1Aff* p1;          // L_i, affine, 2^256 form ((0, 0) = identity)
  const G1Aff* p2;          // -proof_i
  u32 n;
  const Line* lines_a;      // g2's table
  const Line* lines_b;      // [tau]_2's
  Fq* ws;                   // FE_NSLOTS * 12 * ws_n Fq
  size_t ws_n;
  uint8_t* status;          // out: 0 = the equation holds, 1 = it does not
};

// TWO lanes per item. Tail lanes redo the last item and write nothing: all 64 lanes stay active for the DPP exchanges.
// `ell` at P = (0, 0) does not multiply by one, so an item with an identity is decided without the pairing: it is valid iff BOTH points are the
// identity (e(0, .) = 1 on both sides). Control flow stays wave-uniform: such a lane pair runs the arithmetic on the zeros and discards it.
static __global__ void __launch_bounds__(64, 2) k_pairing2(Pair2Args a) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 item = t >> 1;
  const u32 i = item < a.n ? item : (a.n - 1);
  __shared__ uint4 park[PARK_CHUNKS * 64 + 16];     // + 64 words: the lanes' item indices
  item_park(park, i);
  Fq12 f;
  {
    const G1Aff p1 = a.p1[i], p2 = a.p2[i];
    miller_loop2(&f, to261(p1.x), to261(p1.y), to261(p2.x), to261(p2.y), a.lines_a, a.lines_b, park);
  }
  fe_run(&f, a.ws, a.ws_n, park);
  // f == 1: canonical words of c0.c0.c0 (Fq2 coefficient 0, even lane) are (1, 0 .. 0), every other component is zero. The loop runs over LDS,
  // as gt_serialize does: a dynamic index into the register copy of f would send it to scratch memory.
  u32 diff = 0;
  {
    const Fq2d* c = reinterpret_cast<const Fq2d*>(&f);
#pragma unroll
    for (int k = 0; k < 6; k++) park_fq(park, k, c[k].v);
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      u32 w[8];
      canon_words(w, unpark_fq(park, k));
      diff |= w[0] ^ ((k == 0 && lane_odd() == 0) ? 1u : 0u);
#pragma unroll
      for (int j = 1; j < 8; j++) diff |= w[j];
    }
  }
  diff |= (u32)__builtin_amdgcn_update_dpp(0, (int)diff, 0xB1, 0xF, 0xF, true);      // the partner's half of the element
  // the identity rule, from the points read again (flags kept from the kernel's entry to here would be spilled)
  const u32 idx = item_unpark(park);
  const bool inf1 = aff_is_inf(a.p1[idx]), inf2 = aff_is_inf(a.p2[idx]);
  const bool bad = (inf1 || inf2) ? !(inf1 && inf2) : diff != 0;
  // the item index again, from a thread index the compiler cannot connect to the one of the kernel's entry
  u32 tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const u32 item_out = (blockIdx.x * blockDim.x + tid) >> 1;
  if (item_out < a.n && (tid & 1u) == 0) a.status[item_out] = bad ? 1 : 0;
}

// items [0, n) of d_p1 / d_p2 -> d_status, in ONE launch; n <= ws_items, the items the FE slots at d_ws were reserved for
keaki_status pairing2_fixed_run(keaki_hip_ctx* ctx, const void* d_p1, const void* d_p2, size_t n, const void* d_lines_a, const void* d_lines_b, void* d_ws,
                                size_t ws_items, void* d_status) {
  if (n == 0) return KEAKI_OK;
  if (n > ws_items || n > pairing_launch_items()) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing2_fixed: %zu items in a launch with slots for %zu", n, ws_items);
  Pair2Args a;
  a.p1 = (const G1Aff*)d_p1; a.p2 = (const G1Aff*)d_p2; a.n = (u32)n;
  a.lines_a = (const Line*)d_lines_a; a.lines_b = (const Line*)d_lines_b;
  a.ws = (Fq*)d_ws; a.ws_n = ws_items; a.status = (uint8_t*)d_status;
  hipLaunchKernelGGL(k_pairing2, dim3(cdiv(2 * n, 64)), dim3(64), 0, ctx->stream, a);
  return launch_check(ctx, "pairing2_fixed");
}
size_t pairing_slot_bytes() { return (size_t)FE_NSLOTS * 12 * sizeof(Fq); }

}  // namespace keaki_internal
