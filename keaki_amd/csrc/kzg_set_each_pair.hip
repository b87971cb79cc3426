// KZG verify_sets_each, pairing side: valid_i <=> e(A_i, g2) * e(-proof_i, Z2_i) == 1. g2 is fixed for the call, so its line sequence is a table
// (k_g2_prepare: the context's g2gen_lines); Z2_i = [Z_i(tau)]_2 varies per item, so its lines are computed on the fly, as k_pairing computes them.
//   k_pairing2v   route 1. One lane pair per item, as k_pairing (pairing.hip.h), whose device functions run here as they are: a step of the loop over
//                 MILLER_STEPS squares f ONCE, multiplies it by the on-the-fly line of the running point T (started at Z2_i; line_double / line_add exactly as
//                 miller_loop uses them) at -proof_i and by the tabulated line of g2 at A_i -- 64 squarings for the two pairings together -- then ONE final
//                 exponentiation (fe_run) and the comparison with one that k_pairing2 makes: a byte out, not 384.
//                 Park map (pair261.hip.h): T in 0..2, the temporaries of the squaring and the line product in 3..5, -proof_i in 6..7, the item index
//                 directly behind PARK_CHUNKS. A_i has no index left there, so the kernel's LDS array is four chunks longer IN FRONT: A_i waits in those
//                 (SV_FRONT), and everything the shared device functions address -- the item index included -- keeps its offset from `park`.
//   k_sp_points   -proof_i for route 1; for route 2 the 2m pairs of the Miller-loop launch: ps = [A_i : m | -proof_i : m], qs = [g2 : m | Z2_i : m].
//   k_sp_status   route 2: the status byte from the 384 serialised bytes of FE(miller(A_i, g2) miller(-proof_i, Z2_i)) and the identity rule.
// The identity rule (both routes): R = (proof_i is the identity or Z2_i is); with A_i or R an identity the item is valid iff both are. The pairing
// kernels count an identity in either slot as GT one, which decides such an item differently (A_i = 0 with R false would pass), so the rule is applied from the
// points, not from the arithmetic.
// A translation unit of its own: k_pairing's generated code does not depend on these kernels in any way.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this file): k_pairing2v 245 VGPRs, no AGPRs, NO scratch memory (k_pairing: 255 VGPRs, none),
// 22,784 B LDS (k_pairing's 18,688 + the four chunks in front), two waves per SIMD. (With Z2_i's address held in a register pair over the loop the kernel
// spilled 16 B per lane: the address is formed again from the parked item index where the 24 addition steps need it.) k_sp_points 46 VGPRs, k_sp_status 46,
// neither with LDS or scratch memory.
// MEASURED (profiles/set_each_times.txt): the fused kernel LOSES to route 2 at every size but n = 32,768 -- set_rows_plan.h: se_route has the figures -- so
// the plan takes route 2 and this kernel runs only under set_each_route = 1.
#define KEAKI_FQ2_OUTLINE 1
#include "internal.h"
#include "pairing.hip.h"
namespace keaki_internal {
using namespace bn254;

constexpr int SV_FRONT = 4;       // chunks in front of `park`: A_i (two Fq)

// f = prod over the steps of (f^2 if the step squares) * l_T(P2) * l_g2(P1), T walking from Q. Parked: T in 0..2, P2 in 6..7, P1 in front[0..1]; the
// squaring and the line products use 3..5 for their temporaries; while a line function runs f waits in 0..5 and T visits registers (miller_loop).
static KTOWER void miller_loop2v(Fq12* f, const Fq& p1x, const Fq& p1y, const Fq& p2x, const Fq& p2y, const G2Aff* __restrict__ qs, const Line* __restrict__ lines_a,
                                 uint4* park, uint4* front) {
  const u32 par = lane_odd();
  fq12_set_one(f);
  {
    const Fq* qw = reinterpret_cast<const Fq*>(qs + item_unpark(park));
    park_fq(park, 0, to261(qw[par])); park_fq(park, 1, to261(qw[2 + par])); park_fq(park, 2, fq2d_one().v);     // T = (Q.x, Q.y, 1)
  }
  park_fq(park, 6, p2x); park_fq(park, 7, p2y);
  park_fq(front, 0, p1x); park_fq(front, 1, p1y);
#pragma unroll 1
  for (int li = 0; li < MILLER_NSTEPS; li++) {
    const int st = MILLER_STEPS[li];
    if (st == 1) fq12_sqr<true>(f, f, park, 3);
    Line l;
    {
      G2Hom r = {{unpark_fq(park, 0)}, {unpark_fq(park, 1)}, {unpark_fq(park, 2)}};
      {
        const Fq2d* c = reinterpret_cast<const Fq2d*>(f);
#pragma unroll
        for (int k = 0; k < 6; k++) park_fq(park, k, c[k].v);                              // f out of the way of the calls
      }
      if (st <= 1) {
        line_double(&r, &l);
      } else {
        // Q, -Q, pi(Q), -pi^2(Q): read again through the parked item index (a pointer per lane held over the loop is what the compiler spills)
        const Fq* qw = reinterpret_cast<const Fq*>(qs + item_unpark(park));
        Fq2d ax = {to261(qw[par])}, ay = {to261(qw[2 + par])};
        if (st == 3) ay = fq2_neg(ay);
        if (st >= 4) {
          ax = M2(fq2_conj(ax), fq2d_load(&p261::TWIST_MUL_BY_Q_X)); ay = M2(fq2_conj(ay), fq2d_load(&p261::TWIST_MUL_BY_Q_Y));
          if (st == 5) { ax = M2(fq2_conj(ax), fq2d_load(&p261::TWIST_MUL_BY_Q_X)); ay = fq2_neg(M2(fq2_conj(ay), fq2d_load(&p261::TWIST_MUL_BY_Q_Y))); }
        }
        line_add(&r, &ax, &ay, &l);
      }
      {
        Fq2d* c = reinterpret_cast<Fq2d*>(f);
#pragma unroll
        for (int k = 0; k < 6; k++) c[k].v = unpark_fq(park, k);
      }
      park_fq(park, 0, r.x.v); park_fq(park, 1, r.y.v); park_fq(park, 2, r.z.v);
    }
    ell(f, &l, cut(unpark_fq(park, 6)), cut(unpark_fq(park, 7)), park, 3);
    l = lines_a[li * 2 + par];
    ell(f, &l, cut(unpark_fq(front, 0)), cut(unpark_fq(front, 1)), park, 3);
  }
}

struct Pair2vArgs {
  const G1Aff* p1;          // A_i, affine, 2^256 form ((0, 0) = identity)
  const G1Aff* p2;          // -proof_i
  const G2Aff* q;           // Z2_i
  u32 n;
  const Line* lines_a;      // g2's table
  Fq* ws;                   // FE_NSLOTS * 12 * ws_n Fq
  size_t ws_n;
  uint8_t* status;          // out: 0 = the equation holds, 1 = it does not
};

// TWO lanes per item. Tail lanes redo the last item and write nothing: all 64 lanes stay active for the DPP exchanges. Control flow stays wave-uniform:
// a lane pair with an identity runs the arithmetic on the zeros and discards it.
static __global__ void __launch_bounds__(64, 2) k_pairing2v(Pair2vArgs a) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 item = t >> 1;
  const u32 i = item < a.n ? item : (a.n - 1);
  __shared__ uint4 lds[SV_FRONT * 64 + PARK_CHUNKS * 64 + 16];     // front | park | 64 words: the lanes' item indices
  uint4* park = lds + SV_FRONT * 64;
  item_park(park, i);
  Fq12 f;
  {
    const G1Aff p1 = a.p1[i], p2 = a.p2[i];
    miller_loop2v(&f, to261(p1.x), to261(p1.y), to261(p2.x), to261(p2.y), a.q, a.lines_a, park, lds);
  }
  fe_run(&f, a.ws, a.ws_n, park);
  // f == 1, as k_pairing2 tests it: over LDS, so that no dynamic index reaches the register copy of f
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
  const bool inf_a = aff_is_inf(a.p1[idx]), inf_r = aff_is_inf(a.p2[idx]) || aff_is_inf(a.q[idx]);
  const bool bad = (inf_a || inf_r) ? !(inf_a && inf_r) : diff != 0;
  // the item index again, from a thread index the compiler cannot connect to the one of the kernel's entry
  u32 tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const u32 item_out = (blockIdx.x * blockDim.x + tid) >> 1;
  if (item_out < a.n && (tid & 1u) == 0) a.status[item_out] = bad ? 1 : 0;
}

// qs == nullptr: ps[i] = -proof_i. Else ps = [A_i : m | -proof_i : m], qs = [g2 : m | Z2_i : m].
static __global__ void __launch_bounds__(256) k_sp_points(const G1Aff* __restrict__ as, const G1Aff* __restrict__ proofs, const G2Aff* __restrict__ z2, u32 m,
                                                          G1Aff* __restrict__ ps, G2Aff* __restrict__ qs) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const G1Aff proof = proofs[i];
  const G1Aff neg = aff_cneg(proof, !aff_is_inf(proof));
  if (!qs) { ps[i] = neg; return; }
  ps[i] = as[i];
  ps[(size_t)m + i] = neg;
  qs[i].x = G2_GEN_XY[0];
  qs[i].y = G2_GEN_XY[1];
  qs[(size_t)m + i] = z2[i];
}

// gt: 96 words per item, serialize_uncompressed of the product's final exponentiation; GT one = the word 1, then zeros
static __global__ void __launch_bounds__(256) k_sp_status(const u32* __restrict__ gt, const G1Aff* __restrict__ as, const G1Aff* __restrict__ proofs,
                                                          const G2Aff* __restrict__ z2, u32 m, uint8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint4* g = reinterpret_cast<const uint4*>(gt + (size_t)96 * i);
  u32 diff = 0;
#pragma unroll 4
  for (u32 c = 0; c < 24; c++) {
    const uint4 w = g[c];
    diff |= (c == 0 ? w.x ^ 1u : w.x) | w.y | w.z | w.w;
  }
  const bool inf_a = aff_is_inf(as[i]), inf_r = aff_is_inf(proofs[i]) || aff_is_inf(z2[i]);
  status[i] = ((inf_a || inf_r) ? !(inf_a && inf_r) : diff != 0) ? 1 : 0;
}

// items [0, n) -> d_status, in ONE launch; n <= ws_items, the items the FE slots at d_ws were reserved for. d_proofs: the NEGATED proofs.
keaki_status pairing2v_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_neg_proofs, const void* d_z2, size_t n, const void* d_lines_g2, void* d_ws,
                           size_t ws_items, void* d_status) {
  if (n == 0) return KEAKI_OK;
  if (n > ws_items || n > pairing_launch_items()) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing2v: %zu items in a launch with slots for %zu", n, ws_items);
  Pair2vArgs a;
  a.p1 = (const G1Aff*)d_a; a.p2 = (const G1Aff*)d_neg_proofs; a.q = (const G2Aff*)d_z2; a.n = (u32)n;
  a.lines_a = (const Line*)d_lines_g2;
  a.ws = (Fq*)d_ws; a.ws_n = ws_items; a.status = (uint8_t*)d_status;
  hipLaunchKernelGGL(k_pairing2v, dim3(cdiv(2 * n, 64)), dim3(64), 0, ctx->stream, a);
  return launch_check(ctx, "pairing2v");
}

keaki_status set_each_points_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_proofs, const void* d_z2, size_t m, void* d_ps, void* d_qs) {
  if (m == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_sp_points, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, (const G1Aff*)d_a, (const G1Aff*)d_proofs, (const G2Aff*)d_z2, (u32)m,
                     (G1Aff*)d_ps, (G2Aff*)d_qs);
  return launch_check(ctx, "set_each_points");
}

keaki_status set_each_status_run(keaki_hip_ctx* ctx, const void* d_gt_bytes, const void* d_a, const void* d_proofs, const void* d_z2, size_t m, void* d_status) {
  if (m == 0) return KEAKI_OK;
  hipLaunchKernelGGL(k_sp_status, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, (const u32*)d_gt_bytes, (const G1Aff*)d_a, (const G1Aff*)d_proofs,
                     (const G2Aff*)d_z2, (u32)m, (uint8_t*)d_status);
  return launch_check(ctx, "set_each_status");
}

}  // namespace keaki_internal
