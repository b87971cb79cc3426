// libkeaki_hip.so -- the KZG verification family of the C ABI (include/keaki_hip.h, which gives the entries their C linkage): verify, verify_batch,
// verify_cosets, pairing_product, verify_sets, verify_each, the coset / set pairs and their per-item verdicts. Host code only (api.hip, api_host.h).
#include "api_host.h"
#include "host_plan.h"
#include "coset_rows_plan.h"
#include "set_rows_plan.h"

using namespace keaki_internal;

// ---- KZG verify -----------------------------------------------------------------------------------------------------
keaki_status keaki_hip_kzg_verify(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* point,
                                  const uint64_t* value, const uint64_t* proof_aff, int32_t* ok_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify");
  if (!com_aff || !tau_g2_aff || !point || !value || !proof_aff || !ok_out) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_verify: null pointer");
  // The predicate exactly as src/kzg.rs:135-143 writes it: e(com - value g1, g2) == e(proof, [tau]_2 - point g2). Both inner points are fixed-base
  // sums over the 8-bit tables of the generators (k_verify_points, 0.25 ms); the two pairings are ONE launch of the twelve-lane kernel with the
  // lines computed on the fly (1.44 ms). (Rounds 2-4 moved point * proof across the pairing so that both second slots were tabulated: a variable-
  // base ladder of 0.99 ms in front of 1.38 ms of pairings.)
  // io block: [qs: g2 128 | Q 128] [in: com 64 | proof 64 | value 32 | point 32 | tau_g2 128] [ps: A 64 | proof 64] [gt 768]
  constexpr size_t O_Q = 0, O_IN = 256, O_P = O_IN + 320, O_GT = O_P + 128, IO_BYTES = O_GT + 768;
  KemState& k = ctx->kem;
  if (!k.verify_ready) {
    ST_TRY(reserve(ctx, k.verify_io, IO_BYTES));
    ST_TRY(g2_generator_to(ctx, (char*)k.verify_io.p + O_Q));
    k.verify_ready = true;                  // only after every step succeeded (a failed init is retried by the next call)
  }
  char* io = (char*)k.verify_io.p;
  if (!k.verify_tables_ready) {
    ST_TRY(small_g1_table(ctx));
    ST_TRY(small_g2_tables(ctx, io + O_Q));   // shared with the small-batch path of encapsulate (which also keeps [tau]_2's table there)
    k.verify_tables_ready = true;
  }
  uint64_t in[40];
  memcpy(in, com_aff, 64);
  memcpy(in + 8, proof_aff, 64);
  memcpy(in + 16, value, 32);
  memcpy(in + 20, point, 32);
  memcpy(in + 24, tau_g2_aff, 128);
  CopyFeed feed(ctx);                       // declared after `in`: a failing call drains the copy while the array is alive
  ST_TRY(feed.put(0, io + O_IN, in, 320));
  HIP_TRY(ctx, hipMemcpyAsync(io + O_P + 64, io + O_IN + 64, 64, hipMemcpyDeviceToDevice, ctx->stream));      // the proof into the pairing's first slot
  ST_TRY(verify_points_run(ctx, k.fbs_g1_gen.p, k.fbs_g2_gen.p, FB_WB_SMALL, io + O_IN, io + O_IN + 192, io + O_IN + 128, io + O_IN + 160, io + O_P, io + O_Q + 128));
  return feed.closed_by(pair2_verdict(ctx, io + O_P, io + O_Q, io + O_GT, nullptr, ok_out));
}

// ---- KZG batch verification: n openings, one random linear combination, two pairings ------------------------------------------------------
// L = sum gamma_i C_i - (sum gamma_i y_i) g1 + sum (gamma_i z_i) proof_i, R = sum gamma_i proof_i, accept <=> e(L, g2) == e(R, [tau]_2):
// sum gamma_i x (the predicate of src/kzg.rs:135-148 with z_i proof_i moved across the pairing). Kernel sequence, all on ctx->stream:
//   MSM R (gammas over the proofs as an ad-hoc base vector, no tables) | k_vb_prepare + k_vb_finish (s_i = gamma_i z_i, g, -t) | MSM M (s over the
//   proofs) | K: MSM (gammas over the commitments) or g C | (-t) g1 (the same scalar-mult launch as g C) | g1_sum of K, M, (-t) g1 | the two
//   pairings in ONE launch | 768 GT bytes + the two sums back.
// vb_io block: [gt: g 32 | -t 32] [pts: C 64 | g1 64] [mul: g C 64 | (-t) g1 64] [sum_in: K 96 | M 96 | T 96] [L 96] [R 96] [ps: L 64 | R 64]
//              [qs: g2 128 | tau 128] [omega 32] [gt 768] [partials]
namespace {
// The sum block that both combination layouts end in, placed at AT: the three terms of L, the two sums, the pairing's arguments and its result.
//   [sum_in: K 96 | M 96 | T 96] [L 96] [R 96] [ps: L 64 | R 64] [qs: g2 128 | tau 128] [omega 32] [gt 768]
template <size_t AT> struct SumBlock { static constexpr size_t O_SUM = AT, O_L = AT + 288, O_R = AT + 384, O_PS = AT + 480, O_QS = AT + 608, O_OMEGA = AT + 864, O_GT = AT + 896, O_END = AT + 1664; };
// how both combinations finish, `sum` = the block on the device: L = K + M + T, both sums affine, the two pairings and the verdict
keaki_status combination_finish(keaki_hip_ctx* ctx, char* sum, int32_t* ok_out, uint64_t* sums_out_aff) {
  using B = SumBlock<0>;
  ST_TRY(g1_sum_run(ctx, sum, 3, sum + B::O_L));
  ST_TRY(verify_batch_jac_to_aff_run(ctx, sum + B::O_L, sum + B::O_R, sum + B::O_PS));
  return pair2_verdict(ctx, sum + B::O_PS, sum + B::O_QS, sum + B::O_GT, sums_out_aff, ok_out);
}
struct VbLayout : SumBlock<320> { static constexpr size_t O_SC = 0, O_PTS = 64, O_MUL = 192, O_PART = O_END; };
// com_stride and point_mode, the two switches every entry of the family has (`what`: the entry's name)
keaki_status kzg_modes_ok(keaki_hip_ctx* ctx, const char* what, int32_t com_stride, int32_t point_mode) {
  if ((com_stride == 0 || com_stride == 1) && (point_mode == 0 || point_mode == 1)) return KEAKI_OK;
  return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: com_stride = %d, point_mode = %d: both must be 0 or 1", what, (int)com_stride, (int)point_mode);
}
// The ONE argument check of verify_batch and verify_each. `out` / `out_name`: the output required at any n; `arrays_ok`: the call's arrays are there (asked for n > 0).
keaki_status openings_args(keaki_hip_ctx* ctx, const char* what, int32_t com_stride, int32_t point_mode, const void* out, const char* out_name, bool arrays_ok, size_t n) {
  ST_TRY(kzg_modes_ok(ctx, what, com_stride, point_mode));
  if (!out) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: %s is null", what, out_name);
  if (n && !arrays_ok) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: null pointer", what);
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: n must be < 2^31 per device", what);
  return KEAKI_OK;
}
// `stage(phase)`: the host form uploads what the phase reads and makes ctx->stream wait for it (0: gammas and proofs, in front of the first MSM;
// 1: commitments, points, values). The commitment (com_stride 0), [tau]_2 and omega (point_mode 1) are already in their vb_io slots.
keaki_status verify_batch_core(keaki_hip_ctx* ctx, const void* d_coms, int32_t com_stride, const void* d_points, int32_t point_mode, const void* d_values,
                               const void* d_proofs, const void* d_gammas, size_t n, const std::function<keaki_status(int)>& stage, int32_t* ok_out,
                               uint64_t* sums_out_aff) {
  using V = VbLayout;
  char* io = (char*)ctx->vb_io.p;
  ST_TRY(g1_generator_to(ctx, io + V::O_PTS + 64));
  ST_TRY(g2_generator_to(ctx, io + V::O_QS));
  if (stage) ST_TRY(stage(0));
  ST_TRY(msm_g1_run(ctx, d_proofs, n, d_gammas, n, io + V::O_R));
  if (stage) ST_TRY(stage(1));
  ST_TRY(verify_batch_scalars_run(ctx, d_gammas, point_mode ? (const void*)(io + V::O_OMEGA) : d_points, point_mode, d_values, n, ctx->vb_s.p, io + V::O_PART,
                                  io + V::O_SC));
  ST_TRY(msm_g1_run(ctx, d_proofs, n, ctx->vb_s.p, n, io + V::O_SUM + 96));
  if (com_stride) {
    ST_TRY(msm_g1_run(ctx, d_coms, n, d_gammas, n, io + V::O_SUM));
    ST_TRY(g1_mul_batch_run(ctx, io + V::O_PTS + 64, 1, io + V::O_SC + 32, 1, io + V::O_MUL + 64));           // (-t) g1
    ST_TRY(verify_batch_aff_to_jac_run(ctx, io + V::O_MUL + 64, 1, io + V::O_SUM + 192));
  } else {
    ST_TRY(g1_mul_batch_run(ctx, io + V::O_PTS, 1, io + V::O_SC, 2, io + V::O_MUL));                          // g C and (-t) g1, one launch
    ST_TRY(verify_batch_aff_to_jac_run(ctx, io + V::O_MUL, 1, io + V::O_SUM));
    ST_TRY(verify_batch_aff_to_jac_run(ctx, io + V::O_MUL + 64, 1, io + V::O_SUM + 192));
  }
  return combination_finish(ctx, io + V::O_SUM, ok_out, sums_out_aff);
}
// the empty combination: both sums are the identity, which pairs to GT one on both sides
void verify_batch_empty(int32_t* ok_out, uint64_t* sums_out_aff) {
  *ok_out = 1;
  if (sums_out_aff) memset(sums_out_aff, 0, 128);
}
keaki_status verify_batch_reserve(keaki_hip_ctx* ctx, size_t n) {
  ST_TRY(reserve(ctx, ctx->vb_io, VbLayout::O_PART + verify_batch_partials_bytes()));
  return reserve(ctx, ctx->vb_s, n * 32);
}
}  // namespace

keaki_status keaki_hip_kzg_verify_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, int32_t com_stride, const void* d_tau_g2_aff, const void* d_points,
                                            int32_t point_mode, const void* d_values, const void* d_proofs_aff, const void* d_gammas, size_t n,
                                            int32_t* ok_out, uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_batch");
  ST_TRY(openings_args(ctx, "kzg_verify_batch", com_stride, point_mode, ok_out, "ok_out", d_com_aff && d_tau_g2_aff && d_points && d_values && d_proofs_aff && d_gammas, n));
  if (n == 0) { verify_batch_empty(ok_out, sums_out_aff); return KEAKI_OK; }
  ST_TRY(verify_batch_reserve(ctx, n));
  char* io = (char*)ctx->vb_io.p;
  if (!com_stride) HIP_TRY(ctx, hipMemcpyAsync(io + VbLayout::O_PTS, d_com_aff, 64, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(io + VbLayout::O_QS + 128, d_tau_g2_aff, 128, hipMemcpyDeviceToDevice, ctx->stream));
  if (point_mode) HIP_TRY(ctx, hipMemcpyAsync(io + VbLayout::O_OMEGA, d_points, 32, hipMemcpyDeviceToDevice, ctx->stream));
  return verify_batch_core(ctx, d_com_aff, com_stride, d_points, point_mode, d_values, d_proofs_aff, d_gammas, n, nullptr, ok_out, sums_out_aff);
}

keaki_status keaki_hip_kzg_verify_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, int32_t com_stride, const uint64_t* tau_g2_aff, const uint64_t* points,
                                        int32_t point_mode, const uint64_t* values, const uint64_t* proofs_aff, const uint64_t* gammas, size_t n,
                                        int32_t* ok_out, uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);                 // held across stage -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_batch");
  ST_TRY(openings_args(ctx, "kzg_verify_batch", com_stride, point_mode, ok_out, "ok_out", com_aff && tau_g2_aff && points && values && proofs_aff && gammas, n));
  if (n == 0) { verify_batch_empty(ok_out, sums_out_aff); return KEAKI_OK; }
  ST_TRY(verify_batch_reserve(ctx, n));
  ST_TRY(reserve(ctx, ctx->io_a, n * 32));
  ST_TRY(reserve(ctx, ctx->io_d, n * 32));
  char* io = (char*)ctx->vb_io.p;
  ItemStager items{ctx, com_aff, com_stride, io + VbLayout::O_PTS, points, point_mode, io + VbLayout::O_OMEGA, proofs_aff, n};
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);
  ST_TRY(items.put(feed, ItemStager::ONE_COM));
  ST_TRY(feed.put(0, io + VbLayout::O_QS + 128, tau_g2_aff, 128));
  ST_TRY(items.put(feed, ItemStager::OMEGA));
  // Large batches (160 B per item) go up on the context's copy stream in the order the kernels ask for them: gammas and proofs, then -- under
  // the first MSM -- commitments, points and values. Small ones, and a context told to use no other stream (pipe_chunks = 0), copy in front.
  ST_TRY(feed.begin(ctx->tune.pipe_chunks && n >= PIPE_CHUNK));
  const std::function<keaki_status(int)> stage = [&](int phase) -> keaki_status {
    if (phase == 0) {
      ST_TRY(items.put(feed, ctx->io_a.p, gammas, n * 32));
      return items.put(feed, ItemStager::PROOFS);
    }
    ST_TRY(items.put(feed, ItemStager::POINTS));
    ST_TRY(items.put(feed, ctx->io_d.p, values, n * 32));
    return items.put(feed, ItemStager::COMS);
  };
  return feed.closed_by(verify_batch_core(ctx, items.d_com(), com_stride, items.d_points(), point_mode, ctx->io_d.p, items.d_proofs(), ctx->io_a.p, n, stage, ok_out,
                                          sums_out_aff));
}

// ---- KZG coset batch verification: n set proofs over cosets of size l, one linear combination, two pairings ----------------------------------
// L = sum gamma_k C_k - sum_j J_j [tau^j]_1 + sum (gamma_k c_k) proof_k, R = sum gamma_k proof_k, accept <=> e(L, g2) == e(R, [tau^l]_2): sum gamma_k x
// (verify_multi's predicate on the coset h_k <omega_l>, whose Z is X^l - c_k, with c_k proof_k moved across the pairing). Kernel sequence, all on
// ctx->stream, modelled on verify_batch_core: MSM R (gammas over the proofs) | k_vc_prepare + k_vc_transform + k_vc_finish (kzg_cosets.hip: s_k = gamma_k c_k,
// -J, g) | MSM M (s over the proofs) | MSM T (-J over the first l points of the SRS, with the handle's window tables) | K: MSM (gammas over the
// commitments) or g C | g1_sum of K, M, T | the two pairings in ONE launch | 768 GT bytes + the two sums back.
// vc_io block: [pts: C 64] [mul: g C 64] [sum_in: K 96 | M 96 | T 96] [L 96] [R 96] [ps: L 64 | R 64] [qs: g2 128 | tau^l 128] [omega 32] [gt 768]
namespace {
struct VcLayout : SumBlock<128> { static constexpr size_t O_PTS = 0, O_MUL = 64, TOTAL = O_END; };
// the values of n items as ONE span of the caller's array: up to the last value the strides name
inline size_t coset_span(size_t n, size_t l, size_t item_stride, size_t t_stride) { return (n - 1) * item_stride + (l - 1) * t_stride + 1; }
struct VcArgs {
  const keaki_hip_srs_g1* srs;
  const void *com, *tau_l, *points, *values, *proofs, *gammas;
  int32_t com_stride, point_mode;
  size_t item_stride, t_stride, n;
  uint32_t log2l;
  const uint64_t *omega_l_inv, *inv_l;
};
// The commitment (com_stride 0) and [tau^l]_2 are already in their vc_io slots; a.* are device pointers.
keaki_status verify_cosets_core(keaki_hip_ctx* ctx, const VcArgs& a, const VcWork& w, int32_t* ok_out, uint64_t* sums_out_aff) {
  using V = VcLayout;
  char* io = (char*)ctx->vc_io.p;
  const size_t n = a.n, l = (size_t)1 << a.log2l;
  ST_TRY(g2_generator_to(ctx, io + V::O_QS));
  ST_TRY(msm_g1_run(ctx, a.proofs, n, a.gammas, n, io + V::O_R));
  ST_TRY(verify_cosets_scalars_run(ctx, a.gammas, a.points, a.point_mode, a.values, a.item_stride, a.t_stride, a.log2l, a.omega_l_inv, a.inv_l, n, w));
  ST_TRY(msm_g1_run(ctx, a.proofs, n, w.s, n, io + V::O_SUM + 96));
  const auto t1 = srs_tables(a.srs);
  ST_TRY(msm_g1_run(ctx, a.srs->d, a.srs->n, w.neg_j, l, io + V::O_SUM + 192, t1.first, t1.second));
  if (a.com_stride) {
    ST_TRY(msm_g1_run(ctx, a.com, n, a.gammas, n, io + V::O_SUM));
  } else {
    ST_TRY(g1_mul_batch_run(ctx, io + V::O_PTS, 1, w.g, 1, io + V::O_MUL));                                   // g C
    ST_TRY(verify_batch_aff_to_jac_run(ctx, io + V::O_MUL, 1, io + V::O_SUM));
  }
  return combination_finish(ctx, io + V::O_SUM, ok_out, sums_out_aff);
}
// Two values (k, t) != (k', t') of the call share an address iff a item_stride = b t_stride for some 0 <= a < n, 0 <= b < l, not both zero; the
// smallest such pair is (t_stride / g, item_stride / g), g = gcd.
bool verify_cosets_strides_overlap(size_t n, size_t l, size_t item_stride, size_t t_stride) {
  if ((n > 1 && item_stride == 0) || (l > 1 && t_stride == 0)) return true;
  if (n <= 1 || l <= 1) return false;
  size_t g = item_stride, b = t_stride;
  while (b) { const size_t r = g % b; g = b; b = r; }
  return t_stride / g < n && item_stride / g < l;
}
// The ONE argument check of the coset calls (`what`: kzg_verify_cosets, kzg_coset_pairs, kzg_verify_cosets_each). `out_ok` / `out_name`: the output that is
// required at any n; `rest_ok`: the call's own arrays beyond the commitment, the shifts, the values and the two constants are there (asked for n > 0).
keaki_status verify_cosets_args(keaki_hip_ctx* ctx, const VcArgs& a, const char* what, bool out_ok, const char* out_name, bool rest_ok) {
  ST_TRY(kzg_modes_ok(ctx, what, a.com_stride, a.point_mode));
  if (!out_ok || !a.srs) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: %s is null", what, out_ok ? "srs_g1" : out_name);
  if (a.log2l > 31 || ((size_t)1 << a.log2l) > KEAKI_SET_MAX)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: l = 2^%u exceeds KEAKI_SET_MAX = %d", what, a.log2l, (int)KEAKI_SET_MAX);
  const size_t l = (size_t)1 << a.log2l;
  if (a.n && (!a.com || !a.points || !a.values || !a.omega_l_inv || !a.inv_l || !rest_ok)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: null pointer", what);
  if (a.n >= ((size_t)1 << 31) || a.n * l >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: n * l = %zu * %zu must be < 2^31", what, a.n, l);
  if (a.n && verify_cosets_strides_overlap(a.n, l, a.item_stride, a.t_stride))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: under item_stride = %zu, t_stride = %zu two of the %zu x %zu values share an address", what, a.item_stride,
                a.t_stride, a.n, l);
  // the extent (n - 1) item_stride + (l - 1) t_stride stays below 2^48 values (each term below 2^47, checked without forming a product that could wrap): 32 x the
  // extent, the bytes the host form uploads and the kernels' address arithmetic, fits 64 bits with room to spare
  constexpr size_t HALF = (size_t)1 << 47;
  if (a.n && ((a.n > 1 && a.item_stride >= HALF / (a.n - 1)) || (l > 1 && a.t_stride >= HALF / (l - 1))))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: item_stride = %zu, t_stride = %zu put the last of the %zu x %zu values 2^48 or more values behind the first", what,
                a.item_stride, a.t_stride, a.n, l);
  return srs_holds(ctx, a.srs, what, l, "kzg cosets: I has %zu coefficients but the G1 SRS holds %zu points");
}
}  // namespace

keaki_status keaki_hip_kzg_verify_cosets_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride,
                                             const void* d_tau_l_g2_aff, const void* d_points, int32_t point_mode, const void* d_values,
                                             size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l,
                                             const void* d_proofs_aff, const void* d_gammas, size_t n, int32_t* ok_out, uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_cosets");
  const VcArgs a = {srs_g1, d_com_aff, d_tau_l_g2_aff, d_points, d_values, d_proofs_aff, d_gammas, com_stride, point_mode, item_stride, t_stride, n, log2l,
                    omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_verify_cosets", ok_out != nullptr, "ok_out", a.tau_l && a.proofs && a.gammas));
  if (n == 0) { verify_batch_empty(ok_out, sums_out_aff); return KEAKI_OK; }
  ST_TRY(reserve(ctx, ctx->vc_io, VcLayout::TOTAL));
  ST_TRY(reserve(ctx, ctx->vc_work, verify_cosets_work_bytes(n, log2l)));
  char* io = (char*)ctx->vc_io.p;
  if (!com_stride) HIP_TRY(ctx, hipMemcpyAsync(io + VcLayout::O_PTS, d_com_aff, 64, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(io + VcLayout::O_QS + 128, d_tau_l_g2_aff, 128, hipMemcpyDeviceToDevice, ctx->stream));
  return verify_cosets_core(ctx, a, verify_cosets_layout(n, log2l, ctx->vc_work.p), ok_out, sums_out_aff);
}

keaki_status keaki_hip_kzg_verify_cosets(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride,
                                         const uint64_t* tau_l_g2_aff, const uint64_t* points, int32_t point_mode, const uint64_t* values,
                                         size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l,
                                         const uint64_t* proofs_aff, const uint64_t* gammas, size_t n, int32_t* ok_out, uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_cosets");
  VcArgs a = {srs_g1, com_aff, tau_l_g2_aff, points, values, proofs_aff, gammas, com_stride, point_mode, item_stride, t_stride, n, log2l, omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_verify_cosets", ok_out != nullptr, "ok_out", a.tau_l && a.proofs && a.gammas));
  if (n == 0) { verify_batch_empty(ok_out, sums_out_aff); return KEAKI_OK; }
  // the values go up as the one span the strides name, behind the kernels' own workspace; every buffer is reserved before the first copy
  const size_t span = coset_span(n, (size_t)1 << log2l, item_stride, t_stride), work = (verify_cosets_work_bytes(n, log2l) + 255) & ~(size_t)255;
  ST_TRY(reserve(ctx, ctx->vc_io, VcLayout::TOTAL));
  ST_TRY(reserve(ctx, ctx->vc_work, work + span * 32));
  ST_TRY(reserve(ctx, ctx->io_a, n * 32));
  char* io = (char*)ctx->vc_io.p;
  ItemStager items{ctx, com_aff, com_stride, io + VcLayout::O_PTS, points, point_mode, io + VcLayout::O_OMEGA, proofs_aff, n};
  ST_TRY(items.reserve());
  char* d_values = (char*)ctx->vc_work.p + work;
  CopyFeed feed(ctx);
  ST_TRY(items.put(feed, ItemStager::COM));
  ST_TRY(feed.put(0, io + VcLayout::O_QS + 128, tau_l_g2_aff, 128));
  ST_TRY(items.put(feed, ItemStager::PTS));
  ST_TRY(feed.put(0, ctx->io_a.p, gammas, n * 32));
  ST_TRY(items.put(feed, ItemStager::PROOFS));
  ST_TRY(feed.put(0, d_values, values, span * 32));
  a.com = items.d_com(); a.points = items.d_points(); a.values = d_values; a.proofs = items.d_proofs(); a.gammas = ctx->io_a.p;
  return feed.closed_by(verify_cosets_core(ctx, a, verify_cosets_layout(n, log2l, ctx->vc_work.p), ok_out, sums_out_aff));
}

// ---- pairing product: n Miller loops, a GT product tree, ONE final exponentiation ------------------------------------------------------------
// gp_work block: [product 384] [partial products of the first launch] [Miller-loop outputs: 384 per pair]
namespace {
size_t pairing_product_work_bytes(size_t n) { return 384 + gt_product_part_bytes() + n * 384; }
keaki_status pairing_product_args(keaki_hip_ctx* ctx, const void* out, bool arrays_ok, size_t n) {
  if (!out || (n && !arrays_ok)) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing_product: null pointer");
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing_product: n must be < 2^31");
  return KEAKI_OK;
}
// gp_work is reserved for n pairs; everything is a device pointer. Asynchronous on ctx->stream.
keaki_status pairing_product_core(keaki_hip_ctx* ctx, const void* d_g1, const void* d_g2, size_t n, void* d_gt_out) {
  char* wk = (char*)ctx->gp_work.p;
  char* miller = wk + 384 + gt_product_part_bytes();
  if (n) ST_TRY(miller_only_run(ctx, d_g1, d_g2, n, miller));
  ST_TRY(gt_product_run(ctx, miller, n, wk + 384, wk));
  return final_exp_only_run(ctx, wk, 1, d_gt_out);
}
// serialize_uncompressed(GT one): the canonical words of c0.c0.c0 = 1 come first, every other component is zero
bool gt_bytes_are_one(const uint8_t* gt) {
  if (gt[0] != 1) return false;
  for (size_t i = 1; i < 384; i++) if (gt[i]) return false;
  return true;
}
}  // namespace

keaki_status keaki_hip_pairing_product_dev(keaki_hip_ctx* ctx, const void* d_g1_aff, const void* d_g2_aff, size_t n, void* d_gt_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.pairing_product");
  ST_TRY(pairing_product_args(ctx, d_gt_out, d_g1_aff && d_g2_aff, n));
  ST_TRY(reserve(ctx, ctx->gp_work, pairing_product_work_bytes(n)));
  return pairing_product_core(ctx, d_g1_aff, d_g2_aff, n, d_gt_out);
}

keaki_status keaki_hip_pairing_product(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, size_t n, uint8_t* gt_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.pairing_product");
  ST_TRY(pairing_product_args(ctx, gt_out, g1_aff && g2_aff, n));
  ST_TRY(reserve(ctx, ctx->gp_work, pairing_product_work_bytes(n)));
  ST_TRY(reserve(ctx, ctx->io_a, n * G1_AFF_BYTES + 16));
  ST_TRY(reserve(ctx, ctx->io_b, n * G2_AFF_BYTES + 16));
  ST_TRY(reserve(ctx, ctx->io_c, 384));
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, ctx->io_a.p, g1_aff, n * G1_AFF_BYTES));
  ST_TRY(feed.put(0, ctx->io_b.p, g2_aff, n * G2_AFF_BYTES));
  ST_TRY(pairing_product_core(ctx, ctx->io_a.p, ctx->io_b.p, n, ctx->io_c.p));
  return download(feed, gt_out, ctx->io_c.p, 384);
}

// ---- KZG set batch verification: n set proofs over arbitrary sets of k points, one linear combination, k + 1 Miller loops ---------------------
// J_t = sum gamma_i I_(i,t), L = sum gamma_i C_i - sum_t J_t [tau^t]_1 - sum (gamma_i Z_(i,0)) proof_i, R_t = sum (gamma_i Z_(i,t)) proof_i (1 <= t <= k),
// accept <=> e(-L, g2) prod_t e(R_t, [tau^t]_2) == 1: sum gamma_i x (verify_multi's predicate with the coefficients of Z_i moved across the pairing as G1
// scalars, the t = 0 term folded into the left side). Kernel sequence, all on ctx->stream: k_vs_points (point_mode 1) + k_vs_weights + k_vs_polys + k_vs_finish
// (kzg_sets.hip: the k + 1 scalar rows, -J, g) | the batched MSM of the rows over the proofs as an ad-hoc base vector (row 0 -> M, rows 1 .. k -> R_t; rows
// longer than N_BATCH_MAX run row by row inside msm_g1_batch_run) | MSM T (-J over the first k points of the SRS, with the handle's window tables) | K: MSM
// (gammas over the commitments) or g C | g1_sum of K, T, M | k_vs_pairs (the k + 1 sums affine, and -L) | pairing_product_core on (-L, R_1 .. R_k) x (g2,
// [tau]_2 .. [tau^k]_2) | 384 GT bytes + the sums back, the bytes compared with GT one here.
// vs_io block (KP = KEAKI_VERIFY_SETS_K_MAX + 1): [pts: C 64] [mul: g C 64] [sum_in: K 96 | T 96] [rows: M 96 | R_1 .. R_k 96 each: KP x 96] [L 96]
//              [aff: L, R_t: KP x 64] [ps: -L, R_t: KP x 64] [qs: g2, [tau^t]_2: KP x 128] [gt 384]
namespace {
struct VsLayout {
  static constexpr size_t KP = (size_t)KEAKI_VERIFY_SETS_K_MAX + 1;
  static constexpr size_t O_PTS = 0, O_MUL = 64, O_SUM = 128, O_ROWS = O_SUM + 192, O_L = O_ROWS + KP * 96, O_AFF = O_L + 96, O_PS = O_AFF + KP * 64,
                          O_QS = O_PS + KP * 64, O_GT = O_QS + KP * 128, TOTAL = O_GT + 384;
};
struct VsArgs {
  const keaki_hip_srs_g1* srs1;
  const keaki_hip_srs_g2* srs2;
  const void *com, *points, *values, *proofs, *gammas;
  const uint64_t* omega;
  int32_t com_stride, point_mode;
  size_t item_stride, k, n;
  bool no_proofs = false, no_gammas = false;      // arrays the call does not take (set_pairs: neither; verify_sets_each: no gammas)
};
// the points or values of n items as ONE span of the caller's array: up to the last element the stride names
inline size_t sets_span(size_t n, size_t k, size_t item_stride) { return (n - 1) * item_stride + k; }
// The ONE argument check of the set-batch calls; `out`: the output that is required at any n.
keaki_status verify_sets_args(keaki_hip_ctx* ctx, const VsArgs& a, const char* what, const void* out, const char* out_name = "ok_out") {
  ST_TRY(kzg_modes_ok(ctx, what, a.com_stride, a.point_mode));
  if (!out || !a.srs1 || !a.srs2) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: %s is null", what, !out ? out_name : a.srs1 ? "srs_g2" : "srs_g1");
  if (a.k == 0 || a.k > KEAKI_VERIFY_SETS_K_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: k = %zu must be in 1 .. %d", what, a.k, (int)KEAKI_VERIFY_SETS_K_MAX);
  if (a.item_stride < a.k) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: item_stride = %zu is less than k = %zu", what, a.item_stride, a.k);
  if (a.point_mode && !a.omega) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: point_mode 1 needs omega", what);
  if (a.n && (!a.com || !a.points || !a.values || (!a.no_proofs && !a.proofs) || (!a.no_gammas && !a.gammas))) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: null pointer", what);
  if (a.n >= ((size_t)1 << 31) || a.n * a.k >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: n * k = %zu * %zu must be < 2^31", what, a.n, a.k);
  // the extent (n - 1) item_stride + k stays below 2^48 elements (checked without forming a product that could wrap): 32 x the extent, the bytes the host
  // form uploads and the kernels' address arithmetic, fits 64 bits with room to spare
  if (a.n > 1 && a.item_stride >= ((size_t)1 << 47) / (a.n - 1))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: item_stride = %zu puts the last of the %zu items 2^47 or more elements behind the first", what, a.item_stride, a.n);
  ST_TRY(srs_holds(ctx, a.srs2, what, a.k + 1, "kzg sets: Z has %zu coefficients but the G2 SRS holds %zu points"));
  return srs_holds(ctx, a.srs1, what, a.k, "kzg sets: I has %zu coefficients but the G1 SRS holds %zu points");
}
// the empty combination: every sum is the identity, and the empty product is GT one
void verify_sets_empty(int32_t* ok_out, uint64_t* sums_out_aff, size_t k) {
  *ok_out = 1;
  if (sums_out_aff) memset(sums_out_aff, 0, (k + 1) * G1_AFF_BYTES);
}
// every workspace of a call, before its first copy or launch
keaki_status verify_sets_reserve(keaki_hip_ctx* ctx, const VsArgs& a) {
  ST_TRY(reserve(ctx, ctx->vs_io, VsLayout::TOTAL));
  ST_TRY(reserve(ctx, ctx->vs_work, verify_sets_work_bytes(a.n, a.k, a.point_mode)));
  return reserve(ctx, ctx->gp_work, pairing_product_work_bytes(a.k + 1));
}
// The commitment (com_stride 0) is already in its vs_io slot; a.* are device pointers but a.omega.
keaki_status verify_sets_core(keaki_hip_ctx* ctx, const VsArgs& a, int32_t* ok_out, uint64_t* sums_out_aff) {
  using V = VsLayout;
  char* io = (char*)ctx->vs_io.p;
  const size_t n = a.n, k = a.k;
  const VsWork w = verify_sets_layout(n, k, ctx->vs_work.p);
  ST_TRY(verify_sets_scalars_run(ctx, a.gammas, a.points, a.point_mode, a.omega, a.values, a.item_stride, k, n, w));
  ST_TRY(msm_g1_batch_run(ctx, a.proofs, n, nullptr, 0, w.s, n, k + 1, n, io + V::O_ROWS));
  const auto t1 = srs_tables(a.srs1);
  ST_TRY(msm_g1_run(ctx, a.srs1->d, a.srs1->n, w.neg_j, k, io + V::O_SUM + 96, t1.first, t1.second));
  if (a.com_stride) {
    ST_TRY(msm_g1_run(ctx, a.com, n, a.gammas, n, io + V::O_SUM));
  } else {
    ST_TRY(g1_mul_batch_run(ctx, io + V::O_PTS, 1, w.g, 1, io + V::O_MUL));                                   // g C
    ST_TRY(verify_batch_aff_to_jac_run(ctx, io + V::O_MUL, 1, io + V::O_SUM));
  }
  ST_TRY(g1_sum_run(ctx, io + V::O_SUM, 3, io + V::O_L));                                                     // K + T + M: the row M lies behind them
  ST_TRY(verify_sets_pairs_run(ctx, io + V::O_L, io + V::O_ROWS, k, io + V::O_AFF, io + V::O_PS));
  ST_TRY(g2_generator_to(ctx, io + V::O_QS));
  HIP_TRY(ctx, hipMemcpyAsync(io + V::O_QS + G2_AFF_BYTES, (const char*)a.srs2->d + G2_AFF_BYTES, k * G2_AFF_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
  ST_TRY(pairing_product_core(ctx, io + V::O_PS, io + V::O_QS, k + 1, io + V::O_GT));
  uint8_t gt[384];
  if (sums_out_aff) HIP_TRY(ctx, hipMemcpyAsync(sums_out_aff, io + V::O_AFF, (k + 1) * G1_AFF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  ST_TRY(download(ctx, gt, io + V::O_GT, 384));
  *ok_out = gt_bytes_are_one(gt) ? 1 : 0;
  return KEAKI_OK;
}
}  // namespace

keaki_status keaki_hip_kzg_verify_sets_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const void* d_com_aff,
                                           int32_t com_stride, const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values,
                                           size_t item_stride, size_t k, const void* d_proofs_aff, const void* d_gammas, size_t n, int32_t* ok_out,
                                           uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_sets");
  const VsArgs a = {srs_g1, srs_g2, d_com_aff, d_points, d_values, d_proofs_aff, d_gammas, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(verify_sets_args(ctx, a, "kzg_verify_sets", ok_out));
  if (n == 0) { verify_sets_empty(ok_out, sums_out_aff, k); return KEAKI_OK; }
  ST_TRY(verify_sets_reserve(ctx, a));
  if (!com_stride) HIP_TRY(ctx, hipMemcpyAsync((char*)ctx->vs_io.p + VsLayout::O_PTS, d_com_aff, G1_AFF_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
  return verify_sets_core(ctx, a, ok_out, sums_out_aff);
}

keaki_status keaki_hip_kzg_verify_sets(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                       int32_t com_stride, const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values,
                                       size_t item_stride, size_t k, const uint64_t* proofs_aff, const uint64_t* gammas, size_t n, int32_t* ok_out,
                                       uint64_t* sums_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_sets");
  VsArgs a = {srs_g1, srs_g2, com_aff, points, values, proofs_aff, gammas, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(verify_sets_args(ctx, a, "kzg_verify_sets", ok_out));
  if (n == 0) { verify_sets_empty(ok_out, sums_out_aff, k); return KEAKI_OK; }
  // points (or indices) and values go up as the one span the stride names; every buffer is reserved before the first copy
  const size_t span = sets_span(n, k, item_stride), point_bytes = span * (point_mode ? 4 : 32);
  ST_TRY(verify_sets_reserve(ctx, a));
  ST_TRY(reserve(ctx, ctx->io_a, n * 32));
  ST_TRY(reserve(ctx, ctx->io_c, std::max(point_bytes, n * 32)));
  ST_TRY(reserve(ctx, ctx->io_d, span * 32));
  ItemStager items{ctx, com_aff, com_stride, (char*)ctx->vs_io.p + VsLayout::O_PTS, nullptr, 0, nullptr, proofs_aff, n};
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);
  ST_TRY(items.put(feed, ItemStager::COM));
  ST_TRY(items.put(feed, ctx->io_c.p, points, point_bytes));
  ST_TRY(items.put(feed, ctx->io_a.p, gammas, n * 32));
  ST_TRY(items.put(feed, ItemStager::PROOFS));
  ST_TRY(items.put(feed, ctx->io_d.p, values, span * 32));
  a.com = items.d_com(); a.points = ctx->io_c.p; a.values = ctx->io_d.p; a.proofs = items.d_proofs(); a.gammas = ctx->io_a.p;
  return feed.closed_by(verify_sets_core(ctx, a, ok_out, sums_out_aff));
}

// ---- KZG verify_each: n openings, one verdict each ---------------------------------------------------------------------------------------
// L_i = C_i - y_i g1 + z_i proof_i, valid_i <=> e(L_i, g2) e(-proof_i, [tau]_2) == 1: the predicate of src/kzg.rs:135-148 with z_i proof_i moved
// across the pairing, so that BOTH second arguments are fixed for the call and both line sequences are tables (g2's is the context's g2gen_lines,
// [tau]_2's is built on first use and kept until another [tau]_2 arrives). Kernel sequence per launch chunk of at most pairing_launch_items()
// items, all on ctx->stream: k_ve_g1 (L and -proof, kzg_each.hip) | k_pairing2 (kzg_each_pair.hip: one Miller loop over both tables, one final
// exponentiation, one status byte); then k_ve_count over the n bytes. [tau]_2 = identity is decided here: no pairing, valid_i <=> L_i = identity.
// The host form is one upload in front, the kernels, one download of n bytes (+ 64 n with lhs_out_aff), with no chunk pipeline: the inputs are
// at most 192 B per item against >= 140 ns of pairing work (7.1 M pairings/s), a few per cent, which is not worth the stager's machinery.
// ve_io block: [bad2 16] [com 64] [tau 128] [omega 32]
namespace {
struct VeLayout { static constexpr size_t O_BAD = 0, O_COM = 16, O_TAU = 80, O_OMEGA = 208, BYTES = 240; };
void verify_each_empty(uint64_t* n_bad, uint64_t* first_bad) {
  *n_bad = 0;
  if (first_bad) *first_bad = ~0ull;
}
// What a host form with a verdict per item keeps on the device, [status: n B, rounded up to 64 | L: n x 64 B when the caller asked for them], and how it
// goes back once the counters are in, so that the status bytes are final: one download (status and L lie in one buffer, but go to two arrays of the caller).
struct EachOut {
  size_t n, lhs_off, bytes; uint64_t* lhs_host;
  EachOut(size_t n_, uint64_t* lhs) : n(n_), lhs_off((n_ + 63) & ~(size_t)63), bytes(lhs_off + (lhs ? n_ * G1_AFF_BYTES : 0)), lhs_host(lhs) {}
  char* d_lhs(char* out) const { return lhs_host ? out + lhs_off : nullptr; }
};
keaki_status each_result(CopyFeed& feed, const EachOut& r, const char* out, uint8_t* status) {
  prefault_out(feed.ctx, r.lhs_host, r.lhs_host ? r.n * G1_AFF_BYTES : 0);
  if (r.lhs_host) HIP_TRY(feed.ctx, hipMemcpyAsync(r.lhs_host, out + r.lhs_off, r.n * G1_AFF_BYTES, hipMemcpyDeviceToHost, feed.ctx->stream));
  return download(feed, status, out, r.n);
}
// Everything is device memory: d_com / d_tau / d_omega_or_points as the kernels read them, tau_host = the 128 bytes of [tau]_2 (the key of its line
// table). d_lhs: n x 64 B for the L_i, or null (they stay in the chunk's workspace). Ends with the read-back of the counters: synchronises.
keaki_status verify_each_core(keaki_hip_ctx* ctx, const void* d_coms, int32_t com_stride, const void* d_tau, const uint64_t* tau_host, const void* d_points,
                              int32_t point_mode, const void* d_values, const void* d_proofs, size_t n, void* d_status, void* d_lhs, uint64_t* n_bad,
                              uint64_t* first_bad) {
  KemState& k = ctx->kem;
  bool tau_inf = true;
  for (int j = 0; j < 16; j++) tau_inf = tau_inf && tau_host[j] == 0;
  // the launch chunk: the final exponentiation's slots and the two points per item; a refused reservation halves it, down to one wave of items (host_plan.h)
  size_t ch = std::min(n, pairing_launch_items());
  ST_TRY(reserve_shrinking(KEAKI_ERR_OOM, ch, 32, [](size_t c) { return std::max<size_t>(32, ((c + 1) / 2 + 31) & ~(size_t)31); },
    [&](size_t c) {
      const keaki_status st = reserve(ctx, ctx->ve_pts, c * 2 * G1_AFF_BYTES);
      return st == KEAKI_OK && !tau_inf ? reserve(ctx, ctx->pair_ws, c * pairing_slot_bytes()) : st;
    }, [&] { ctx->err.clear(); }));
  ST_TRY(generator_tables(ctx, false));               // g2's line sequence
  if (!k.fb_ready) ST_TRY(small_g1_table(ctx));
  if (!tau_inf && !k.tau_lines.holds(tau_host)) {
    k.tau_lines.invalidate();
    ST_TRY(reserve(ctx, k.tau_lines.buf, g2_prepared_bytes()));
    ST_TRY(g2_prepare_run(ctx, d_tau, k.tau_lines.buf.p));
    k.tau_lines.publish(tau_host, 0);
  }
  char* io = (char*)ctx->ve_io.p;
  BadTally tally{ctx, io + VeLayout::O_BAD};
  ST_TRY(tally.begin());
  const void* tab_g1 = (k.fb_ready ? k.fb_g1_gen : k.fbs_g1_gen).p;
  const uint32_t wb = k.fb_ready ? FB_WB_LONG : FB_WB_SMALL;
  char* pts = (char*)ctx->ve_pts.p;
  for (size_t lo = 0; lo < n; lo += ch) {
    const size_t m = std::min(ch, n - lo);
    void* lhs = d_lhs ? (char*)d_lhs + lo * G1_AFF_BYTES : pts;
    void* neg = pts + ch * G1_AFF_BYTES;
    ST_TRY(verify_each_g1_run(ctx, d_coms, com_stride, tab_g1, wb, d_points, point_mode, d_values, d_proofs, lo, m, lhs, neg));
    if (tau_inf)
      ST_TRY(verify_each_tau_inf_run(ctx, lhs, m, (char*)d_status + lo));
    else
      ST_TRY(pairing2_fixed_run(ctx, lhs, neg, m, k.g2gen_lines.p, k.tau_lines.buf.p, ctx->pair_ws.p, ch, (char*)d_status + lo));
  }
  ST_TRY(verify_each_count_run(ctx, d_status, n, io + VeLayout::O_BAD));
  return tally.end(n_bad, first_bad);
}
}  // namespace

keaki_status keaki_hip_kzg_verify_each_dev(keaki_hip_ctx* ctx, const void* d_com_aff, int32_t com_stride, const void* d_tau_g2_aff, const void* d_points,
                                           int32_t point_mode, const void* d_values, const void* d_proofs_aff, size_t n, void* d_status, uint64_t* n_bad,
                                           uint64_t* first_bad, void* d_lhs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_each");
  ST_TRY(openings_args(ctx, "kzg_verify_each", com_stride, point_mode, n_bad, "n_bad", d_com_aff && d_tau_g2_aff && d_points && d_values && d_proofs_aff && d_status, n));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  ST_TRY(reserve(ctx, ctx->ve_io, VeLayout::BYTES));
  uint64_t tau_host[16];
  ST_TRY(read_constants(ctx, d_tau_g2_aff, nullptr, tau_host, nullptr));          // the key of the line table
  return verify_each_core(ctx, d_com_aff, com_stride, d_tau_g2_aff, tau_host, d_points, point_mode, d_values, d_proofs_aff, n, d_status, d_lhs_out_aff, n_bad,
                          first_bad);
}

keaki_status keaki_hip_kzg_verify_each(keaki_hip_ctx* ctx, const uint64_t* com_aff, int32_t com_stride, const uint64_t* tau_g2_aff, const uint64_t* points,
                                       int32_t point_mode, const uint64_t* values, const uint64_t* proofs_aff, size_t n, uint8_t* status, uint64_t* n_bad,
                                       uint64_t* first_bad, uint64_t* lhs_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_each");
  ST_TRY(openings_args(ctx, "kzg_verify_each", com_stride, point_mode, n_bad, "n_bad", com_aff && tau_g2_aff && points && values && proofs_aff && status, n));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  const EachOut r(n, lhs_out_aff);
  ST_TRY(reserve(ctx, ctx->ve_io, VeLayout::BYTES));
  ST_TRY(reserve(ctx, ctx->ve_out, r.bytes));
  ST_TRY(reserve(ctx, ctx->io_d, n * 32));
  char* io = (char*)ctx->ve_io.p;
  ItemStager items{ctx, com_aff, com_stride, io + VeLayout::O_COM, points, point_mode, io + VeLayout::O_OMEGA, proofs_aff, n};
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);             // one upload in front, on the context's stream; a failing call drains it before it returns
  ST_TRY(feed.put(0, io + VeLayout::O_TAU, tau_g2_aff, 128));
  ST_TRY(items.put(feed, ItemStager::COM | ItemStager::PTS));
  ST_TRY(feed.put(0, ctx->io_d.p, values, n * 32));
  ST_TRY(items.put(feed, ItemStager::PROOFS));
  char* out = (char*)ctx->ve_out.p;
  ST_TRY(verify_each_core(ctx, items.d_com(), com_stride, io + VeLayout::O_TAU, tau_g2_aff, items.d_points(), point_mode, ctx->io_d.p, items.d_proofs(), n, out, r.d_lhs(out), n_bad, first_bad));
  return each_result(feed, r, out, status);
}

// ---- KZG coset pairs and per-coset verdicts ------------------------------------------------------------------------------------------------
// coset_pairs: A_k = C_k - [I_k(tau)]_1 and c_k = h_k^l for n cosets (kzg_coset_pairs.hip has the derivation and the kernels). Kernel sequence, all on
// ctx->stream: k_vc_prepare<., true> over the n items (c, 1 / h) | per launch chunk (coset_rows_plan.h): k_vc_transform<., true> (the rows), then route 1
// k_cp_rows over the handle's window table, or route 2 msm_g1_batch_run over the rows + k_cp_join; k_cp_affine. verify_cosets_each is coset_pairs into
// cp_pairs [A: n x 64 | c: n x 32 | zeros: n x 32] and verify_each_core on (coms := A, points := c, values := 0, [tau]_2 := [tau^l]_2).
namespace {
keaki_status coset_table_ensure(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2l, uint32_t wb) {
  return srs_cache_ensure(ctx, srs, srs->cr, (int)log2l, (int)wb, cr_table_bytes(log2l, wb), [&](void* t) { return coset_table_run(ctx, srs->d, log2l, wb, t); });
}
// The G1 row sums that coset_pairs and set_pairs share: per item, the commitment joined with the sum of its row of scalars over the first 2^log2l points of
// the handle, affine. Route 1 is k_cp_rows over the handle's window table, route 2 msm_g1_batch_run + k_cp_join; k_cp_affine ends both. The caller holds srs->mu.
struct G1RowSums {
  keaki_hip_ctx* ctx = nullptr; keaki_hip_srs_g1* srs = nullptr;
  uint32_t log2l = 0, wb = 0; int route = 2;
  std::pair<const void*, int> tb{nullptr, 0};
  // the route and the table's width; the table is built here, optional memory like an MSM's window tables (refused: route 2). `table_possible`: the handle holds 2^log2l points
  keaki_status choose(keaki_hip_ctx* c, keaki_hip_srs_g1* s, uint32_t log2l_, bool table_possible) {
    ctx = c; srs = s; log2l = log2l_;
    route = table_possible ? cr_route(ctx->tune.coset_rows_route, log2l) : 2;
    wb = ctx->tune.coset_rows_wb ? (uint32_t)ctx->tune.coset_rows_wb : cr_wb(log2l);
    if (route == 1) {
      const keaki_status st = coset_table_ensure(ctx, srs, log2l, wb);
      if (st == KEAKI_ERR_OOM) { ctx->err.clear(); route = 2; }
      else if (st != KEAKI_OK) return st;
    }
    tb = srs_tables(srs);
    return KEAKI_OK;
  }
  // items [lo, lo + m) of the call: `rows` = the chunk's m rows, `stride` scalars apart, of which the first `used` are read; xyzz (m x 128 B) and jac (route 2:
  // m x 96 B) are the chunk's scratch, d_out takes its m affine points
  keaki_status run(const void* rows, size_t used, size_t stride, const void* com, int32_t com_stride, size_t lo, size_t m, void* xyzz, void* jac, void* d_out) const {
    if (route == 1) {
      ST_TRY(coset_rows_table_run(ctx, srs->cr.p, wb, rows, log2l, cr_slices(m, log2l, (uint64_t)ctx->tune.coset_rows_min_lanes), com, com_stride, lo, m, xyzz));
    } else {
      ST_TRY(msm_g1_batch_run(ctx, srs->d, srs->n, tb.first, tb.second, rows, used, m, stride, jac));
      ST_TRY(coset_rows_join_run(ctx, jac, com, com_stride, lo, m, xyzz));
    }
    return coset_rows_affine_run(ctx, xyzz, m, d_out);
  }
};
// a.* are device pointers; the caller holds the context. Every allocation that can be refused (the table, the workspace) comes before the first launch.
keaki_status coset_pairs_core(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const VcArgs& a, void* d_lhs, void* d_c) {
  const size_t n = a.n, l = (size_t)1 << a.log2l;
  std::lock_guard<std::recursive_mutex> hl(srs->mu);       // the table belongs to the handle: one call per handle at a time
  G1RowSums g1;
  ST_TRY(g1.choose(ctx, srs, a.log2l, true));
  const size_t hinv_bytes = (n * 32 + 255) & ~(size_t)255, per_item = l * 32 + sizeof(uint64_t) * 16 + (g1.route == 2 ? G1_JAC_BYTES : 0);
  size_t ch = cr_chunk_items(n, a.log2l);
  ST_TRY(reserve_shrinking(KEAKI_ERR_OOM, ch, 1, cr_chunk_halve, [&](size_t c) { return reserve(ctx, ctx->cp_work, hinv_bytes + c * per_item); }, [&] { ctx->err.clear(); }));
  char* hinv = (char*)ctx->cp_work.p;
  char* rows = hinv + hinv_bytes;
  char* xyzz = rows + ch * l * 32;
  char* jac = xyzz + ch * 128;
  ST_TRY(coset_pairs_shifts_run(ctx, a.points, a.point_mode, a.log2l, n, d_c, hinv));
  for (size_t lo = 0; lo < n; lo += ch) {
    const size_t m = std::min(ch, n - lo);
    ST_TRY(coset_pairs_rows_run(ctx, a.values, a.item_stride, a.t_stride, hinv, a.log2l, a.omega_l_inv, a.inv_l, lo, m, g1.route == 2, rows));
    ST_TRY(g1.run(rows, l, l, a.com, a.com_stride, lo, m, xyzz, jac, (char*)d_lhs + lo * G1_AFF_BYTES));
  }
  return KEAKI_OK;
}
struct CpPairs { char *a, *c, *zeros; };
keaki_status coset_each_reserve(keaki_hip_ctx* ctx, size_t n, size_t extra, CpPairs* out) {
  ST_TRY(reserve(ctx, ctx->ve_io, VeLayout::BYTES));
  ST_TRY(reserve(ctx, ctx->cp_pairs, n * 128 + extra));
  out->a = (char*)ctx->cp_pairs.p; out->c = out->a + n * G1_AFF_BYTES; out->zeros = out->c + n * 32;
  return KEAKI_OK;
}
keaki_status coset_each_core(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const VcArgs& a, const uint64_t* tau_host, const CpPairs& w, void* d_status, void* d_lhs,
                             uint64_t* n_bad, uint64_t* first_bad) {
  ST_TRY(coset_pairs_core(ctx, srs, a, w.a, w.c));
  HIP_TRY(ctx, hipMemsetAsync(w.zeros, 0, a.n * 32, ctx->stream));
  return verify_each_core(ctx, w.a, 1, a.tau_l, tau_host, w.c, 0, w.zeros, a.proofs, a.n, d_status, d_lhs, n_bad, first_bad);
}
}  // namespace

keaki_status keaki_hip_srs_g1_precompute_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2l) {
  CTX_GUARD(ctx);
  if (!srs || log2l > 31 || ((size_t)1 << log2l) > KEAKI_SET_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g1_precompute_cosets: bad argument");
  ST_TRY(srs_holds(ctx, srs, "srs_g1_precompute_cosets", (size_t)1 << log2l, "kzg cosets: I has %zu coefficients but the G1 SRS holds %zu points"));
  std::lock_guard<std::recursive_mutex> hl(srs->mu);
  return coset_table_ensure(ctx, srs, log2l, cr_wb(log2l));
}

keaki_status keaki_hip_kzg_coset_pairs_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride, const void* d_points,
                                           int32_t point_mode, const void* d_values, size_t item_stride, size_t t_stride, uint32_t log2l,
                                           const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, void* d_lhs_out_aff, void* d_c_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_coset_pairs");
  const VcArgs a = {srs_g1, d_com_aff, nullptr, d_points, d_values, nullptr, nullptr, com_stride, point_mode, item_stride, t_stride, n, log2l, omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_coset_pairs", true, "", d_lhs_out_aff && d_c_out));
  if (n == 0) return KEAKI_OK;
  return coset_pairs_core(ctx, srs_g1, a, d_lhs_out_aff, d_c_out);
}

keaki_status keaki_hip_kzg_coset_pairs(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride, const uint64_t* points,
                                       int32_t point_mode, const uint64_t* values, size_t item_stride, size_t t_stride, uint32_t log2l,
                                       const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, uint64_t* lhs_out_aff, uint64_t* c_out) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_coset_pairs");
  VcArgs a = {srs_g1, com_aff, nullptr, points, values, nullptr, nullptr, com_stride, point_mode, item_stride, t_stride, n, log2l, omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_coset_pairs", true, "", lhs_out_aff && c_out));
  if (n == 0) return KEAKI_OK;
  const size_t span = coset_span(n, (size_t)1 << log2l, item_stride, t_stride);
  ST_TRY(reserve(ctx, ctx->cp_pairs, n * 96));
  ST_TRY(reserve(ctx, ctx->cp_in, span * 32));
  ItemStager items{ctx, com_aff, com_stride, nullptr, points, point_mode, nullptr, nullptr, n};      // one commitment and omega: in io_e and io_c
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);
  ST_TRY(items.put(feed, ItemStager::ALL));
  ST_TRY(feed.put(0, ctx->cp_in.p, values, span * 32));
  a.com = items.d_com(); a.points = items.d_points(); a.values = ctx->cp_in.p;
  char* out = (char*)ctx->cp_pairs.p;
  ST_TRY(coset_pairs_core(ctx, srs_g1, a, out, out + n * G1_AFF_BYTES));
  HIP_TRY(ctx, hipMemcpyAsync(lhs_out_aff, out, n * G1_AFF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, c_out, out + n * G1_AFF_BYTES, n * 32);
}

keaki_status keaki_hip_kzg_verify_cosets_each_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride,
                                                  const void* d_tau_l_g2_aff, const void* d_points, int32_t point_mode, const void* d_values,
                                                  size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv,
                                                  const uint64_t* inv_l, const void* d_proofs_aff, size_t n, void* d_status, uint64_t* n_bad,
                                                  uint64_t* first_bad, void* d_lhs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_cosets_each");
  const VcArgs a = {srs_g1, d_com_aff, d_tau_l_g2_aff, d_points, d_values, d_proofs_aff, nullptr, com_stride, point_mode, item_stride, t_stride, n, log2l,
                    omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_verify_cosets_each", n_bad != nullptr, "n_bad", d_tau_l_g2_aff && d_proofs_aff && d_status));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  CpPairs w;
  ST_TRY(coset_each_reserve(ctx, n, 0, &w));
  uint64_t tau_host[16];
  ST_TRY(read_constants(ctx, d_tau_l_g2_aff, nullptr, tau_host, nullptr));          // the key of the line table
  return coset_each_core(ctx, srs_g1, a, tau_host, w, d_status, d_lhs_out_aff, n_bad, first_bad);
}

keaki_status keaki_hip_kzg_verify_cosets_each(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride,
                                              const uint64_t* tau_l_g2_aff, const uint64_t* points, int32_t point_mode, const uint64_t* values,
                                              size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l,
                                              const uint64_t* proofs_aff, size_t n, uint8_t* status, uint64_t* n_bad, uint64_t* first_bad,
                                              uint64_t* lhs_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_cosets_each");
  VcArgs a = {srs_g1, com_aff, tau_l_g2_aff, points, values, proofs_aff, nullptr, com_stride, point_mode, item_stride, t_stride, n, log2l, omega_l_inv, inv_l};
  ST_TRY(verify_cosets_args(ctx, a, "kzg_verify_cosets_each", n_bad != nullptr, "n_bad", tau_l_g2_aff && proofs_aff && status));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  const size_t span = coset_span(n, (size_t)1 << log2l, item_stride, t_stride);
  const EachOut r(n, lhs_out_aff);
  CpPairs w;
  ST_TRY(coset_each_reserve(ctx, n, r.bytes, &w));
  ST_TRY(reserve(ctx, ctx->cp_in, span * 32));
  ItemStager items{ctx, com_aff, com_stride, nullptr, points, point_mode, nullptr, proofs_aff, n};   // one commitment and omega: in io_e and io_c
  ST_TRY(items.reserve());
  char* io = (char*)ctx->ve_io.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, io + VeLayout::O_TAU, tau_l_g2_aff, 128));
  ST_TRY(items.put(feed, ItemStager::ALL));
  ST_TRY(feed.put(0, ctx->cp_in.p, values, span * 32));
  a.com = items.d_com(); a.tau_l = io + VeLayout::O_TAU; a.points = items.d_points(); a.values = ctx->cp_in.p; a.proofs = items.d_proofs();
  char* out = w.zeros + n * 32;
  ST_TRY(coset_each_core(ctx, srs_g1, a, tau_l_g2_aff, w, out, r.d_lhs(out), n_bad, first_bad));
  return each_result(feed, r, out, status);
}

// ---- KZG set pairs and per-set verdicts --------------------------------------------------------------------------------------------------------
// set_pairs: A_i = C_i - [I_i(tau)]_1 and Z2_i = [Z_i(tau)]_2 for n items of k arbitrary points (kzg_set_pairs.hip has the derivation and the G2 kernels). Kernel
// sequence per launch chunk (set_rows_plan.h), all on ctx->stream: k_vs_points (point_mode 1) + k_vs_weights + k_vs_polys<1 / 2> (kzg_sets.hip: the rows -I padded
// to kp and Z) | G1: coset_pairs' group side at log2l = log2 kp -- k_cp_rows over the G1 handle's window table, or msm_g1_batch_run + k_cp_join -- and k_cp_affine |
// G2: k_sp_rows_g2 over the G2 handle's window table, k_sp_affine_g2. verify_sets_each is set_pairs into sp_pairs [A: n x 64 | Z2: n x 128 | status | the chunk
// block of the pairing side] (or into the caller's arrays), then per launch chunk route 1 k_sp_points (-proof) + k_pairing2v, or route 2 k_sp_points + the Miller
// loops of the 2m pairs + k_gt_pair_product + the final exponentiation + k_sp_status; then k_ve_count.
namespace {
// The argument check of the set-pairs calls: the family's gate, told which arrays these calls do not take. `out`: an output required at any n.
keaki_status set_pairs_args(keaki_hip_ctx* ctx, VsArgs a, const char* what, bool with_proofs, const void* out, const char* out_name) {
  a.no_gammas = true;
  a.no_proofs = !with_proofs;
  return verify_sets_args(ctx, a, what, out, out_name);
}
// afterwards srs->sr.p is the table over at least k bases and *wb_out its width; the caller holds srs->mu. A resident table that covers k is used at its
// width unless set_rows_wb names another; a refused table falls to the next narrower width.
keaki_status set_table_ensure(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs, size_t k, uint32_t* wb_out) {
  SrsCache& c = srs->sr;
  const uint32_t opt = (uint32_t)ctx->tune.set_rows_wb;
  if (c.p && c.key[0] >= (int)k && (opt == 0 || c.key[1] == (int)opt)) { *wb_out = (uint32_t)c.key[1]; return KEAKI_OK; }
  for (uint32_t wb = opt ? opt : sr_wb(k); wb; wb = sr_wb_narrower(wb)) {
    const keaki_status st = srs_cache_ensure(ctx, srs, c, (int)k, (int)wb, sr_table_bytes(k, wb), [&](void* t) { return g2_fb_tables_run(ctx, srs->d, (uint32_t)k, t, wb); });
    if (st == KEAKI_OK) { *wb_out = wb; return KEAKI_OK; }
    if (st != KEAKI_ERR_OOM) return st;
    ctx->err.clear();
  }
  return fail(ctx, KEAKI_ERR_OOM, "kzg_set_pairs: the window table over the first %zu G2 points was refused at every width", k);
}
// a.* are device pointers but a.omega; the caller holds the context. Every allocation that can be refused (the tables, the workspace) comes before the first
// launch that writes an output.
keaki_status set_pairs_core(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs1, keaki_hip_srs_g2* srs2, const VsArgs& a, void* d_lhs, void* d_z2) {
  const size_t n = a.n, k = a.k;
  const uint32_t log2kp = sr_log2kp(k);
  const size_t kp = (size_t)1 << log2kp;
  std::lock_guard<std::recursive_mutex> hl1(srs1->mu);     // the tables belong to the handles: one call per handle at a time
  std::lock_guard<std::recursive_mutex> hl2(srs2->mu);
  G1RowSums g1;
  ST_TRY(g1.choose(ctx, srs1, log2kp, kp <= srs1->n));      // kp > len(srs_g1) >= k: no table over kp points
  uint32_t wb2 = 0;
  ST_TRY(set_table_ensure(ctx, srs2, k, &wb2));
  const size_t per_item = sr_item_bytes(k, log2kp, a.point_mode, g1.route == 2);
  size_t ch = sr_chunk_items(n, log2kp);
  ST_TRY(reserve_shrinking(KEAKI_ERR_OOM, ch, 1, sr_chunk_halve, [&](size_t c) { return reserve(ctx, ctx->sp_work, c * per_item); }, [&] { ctx->err.clear(); }));
  char* w = (char*)ctx->sp_work.p;
  char* pts = w + ch * k * 32;
  char* rows_i = pts + (a.point_mode ? ch * k * 32 : 0);
  char* rows_z = rows_i + ch * kp * 32;
  char* xyzz1 = rows_z + ch * k * 32;
  char* xyzz2 = xyzz1 + ch * 128;
  char* jac = xyzz2 + ch * 256;
  const char* tau_k = (const char*)srs2->d + k * G2_AFF_BYTES;
  for (size_t lo = 0; lo < n; lo += ch) {
    const size_t m = std::min(ch, n - lo);
    ST_TRY(set_pairs_rows_run(ctx, a.points, a.point_mode, a.omega, a.values, a.item_stride, k, lo, m, g1.route == 2, w, pts, rows_i, rows_z));
    ST_TRY(g1.run(rows_i, k, kp, a.com, a.com_stride, lo, m, xyzz1, jac, (char*)d_lhs + lo * G1_AFF_BYTES));
    ST_TRY(set_rows_g2_run(ctx, srs2->sr.p, wb2, rows_z, k, sr_slices(m, log2kp, (uint64_t)ctx->tune.set_rows_min_lanes), tau_k, m, xyzz2));
    ST_TRY(set_rows_affine_g2_run(ctx, xyzz2, m, (char*)d_z2 + lo * G2_AFF_BYTES));
  }
  return KEAKI_OK;
}
// sp_pairs of verify_sets_each: [A: n x 64 | Z2: n x 128 | status: n B rounded up to 64 (host form) | the chunk block]; `ch` = the items of a pairing launch chunk
struct SeWork { char *a, *z2, *status, *chunk; size_t ch; bool route2; };
keaki_status set_each_reserve(keaki_hip_ctx* ctx, size_t n, bool host_form, SeWork* out) {
  const bool route2 = se_route(ctx->tune.set_each_route, n) == 2;
  const size_t fixed = n * (G1_AFF_BYTES + G2_AFF_BYTES) + (host_form ? (n + 63) & ~(size_t)63 : 0);
  ST_TRY(reserve(ctx, ctx->ve_io, VeLayout::BYTES));
  size_t ch = se_chunk_items(n, pairing_launch_items());
  ST_TRY(reserve_shrinking(KEAKI_ERR_OOM, ch, SE_CHUNK_MIN, se_chunk_halve,
    [&](size_t c) {
      const keaki_status st = reserve(ctx, ctx->sp_pairs, fixed + c * se_item_bytes(route2));
      return st == KEAKI_OK ? reserve(ctx, ctx->pair_ws, c * pairing_slot_bytes()) : st;
    }, [&] { ctx->err.clear(); }));
  out->a = (char*)ctx->sp_pairs.p; out->z2 = out->a + n * G1_AFF_BYTES; out->status = out->z2 + n * G2_AFF_BYTES;
  out->chunk = (char*)ctx->sp_pairs.p + fixed; out->ch = ch; out->route2 = route2;
  return KEAKI_OK;
}
// a.* are device pointers but a.omega. d_lhs / d_z2: where the pairs go (the caller's arrays or sp_pairs). Ends with the read-back of the counters: synchronises.
keaki_status set_each_core(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs1, keaki_hip_srs_g2* srs2, const VsArgs& a, const SeWork& w, void* d_lhs, void* d_z2,
                           void* d_status, uint64_t* n_bad, uint64_t* first_bad) {
  const size_t n = a.n, ch = w.ch;
  if (!w.route2) ST_TRY(generator_tables(ctx, false));               // g2's line sequence
  ST_TRY(set_pairs_core(ctx, srs1, srs2, a, d_lhs, d_z2));
  char* io = (char*)ctx->ve_io.p;
  BadTally tally{ctx, io + VeLayout::O_BAD};
  ST_TRY(tally.begin());
  for (size_t lo = 0; lo < n; lo += ch) {
    const size_t m = std::min(ch, n - lo);
    const char* as = (const char*)d_lhs + lo * G1_AFF_BYTES;
    const char* zs = (const char*)d_z2 + lo * G2_AFF_BYTES;
    const char* proofs = (const char*)a.proofs + lo * G1_AFF_BYTES;
    char* status = (char*)d_status + lo;
    if (!w.route2) {
      ST_TRY(set_each_points_run(ctx, as, proofs, zs, m, w.chunk, nullptr));
      ST_TRY(pairing2v_run(ctx, as, w.chunk, zs, m, ctx->kem.g2gen_lines.p, ctx->pair_ws.p, ch, status));
    } else {
      char* ps = w.chunk;
      char* qs = ps + ch * 2 * G1_AFF_BYTES;
      char* mil = qs + ch * 2 * G2_AFF_BYTES;
      char* prod = mil + ch * 768;
      char* gt = prod + ch * 384;
      ST_TRY(set_each_points_run(ctx, as, proofs, zs, m, ps, qs));
      ST_TRY(miller_only_run(ctx, ps, qs, 2 * m, mil));
      ST_TRY(gt_pair_product_run(ctx, mil, mil + m * 384, m, prod));
      ST_TRY(final_exp_only_run(ctx, prod, m, gt));
      ST_TRY(set_each_status_run(ctx, gt, as, proofs, zs, m, status));
    }
  }
  ST_TRY(verify_each_count_run(ctx, d_status, n, io + VeLayout::O_BAD));
  return tally.end(n_bad, first_bad);
}
// the host forms' inputs: the spans of points (or indices) and values in sp_in, the commitments and the proofs through the family's stager
struct SetHostIn {
  size_t point_bytes, value_bytes, value_off;
  SetHostIn(const VsArgs& a) : point_bytes(sets_span(a.n, a.k, a.item_stride) * (a.point_mode ? 4 : 32)), value_bytes(sets_span(a.n, a.k, a.item_stride) * 32),
                               value_off((point_bytes + 255) & ~(size_t)255) {}
  keaki_status reserve(keaki_hip_ctx* ctx) const { return keaki_internal::reserve(ctx, ctx->sp_in, value_off + value_bytes); }
  // uploads everything and turns a's pointers into device pointers
  keaki_status put(keaki_hip_ctx* ctx, CopyFeed& feed, ItemStager& items, VsArgs& a) const {
    char* in = (char*)ctx->sp_in.p;
    ST_TRY(items.put(feed, ItemStager::COM));
    ST_TRY(items.put(feed, in, a.points, point_bytes));
    ST_TRY(items.put(feed, in + value_off, a.values, value_bytes));
    ST_TRY(items.put(feed, ItemStager::PROOFS));
    a.com = items.d_com(); a.points = in; a.values = in + value_off; a.proofs = items.d_proofs();
    return KEAKI_OK;
  }
};
}  // namespace

keaki_status keaki_hip_srs_g2_precompute_sets(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs, size_t k_max) {
  CTX_GUARD(ctx);
  if (!srs || k_max == 0 || k_max > KEAKI_VERIFY_SETS_K_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g2_precompute_sets: bad argument");
  ST_TRY(srs_holds(ctx, srs, "srs_g2_precompute_sets", k_max + 1, "kzg sets: Z has %zu coefficients but the G2 SRS holds %zu points"));
  std::lock_guard<std::recursive_mutex> hl(srs->mu);
  uint32_t wb = 0;
  return set_table_ensure(ctx, srs, k_max, &wb);
}

keaki_status keaki_hip_kzg_set_pairs_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const void* d_com_aff, int32_t com_stride,
                                         const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values, size_t item_stride, size_t k,
                                         size_t n, void* d_lhs_out_aff, void* d_z2_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_set_pairs");
  const VsArgs a = {srs_g1, srs_g2, d_com_aff, d_points, d_values, nullptr, nullptr, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(set_pairs_args(ctx, a, "kzg_set_pairs", false, n == 0 || (d_lhs_out_aff && d_z2_out_aff) ? (const void*)ctx : nullptr, "lhs_out_aff or z2_out_aff"));
  if (n == 0) return KEAKI_OK;
  return set_pairs_core(ctx, srs_g1, srs_g2, a, d_lhs_out_aff, d_z2_out_aff);
}

keaki_status keaki_hip_kzg_set_pairs(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff, int32_t com_stride,
                                     const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values, size_t item_stride, size_t k,
                                     size_t n, uint64_t* lhs_out_aff, uint64_t* z2_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_set_pairs");
  VsArgs a = {srs_g1, srs_g2, com_aff, points, values, nullptr, nullptr, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(set_pairs_args(ctx, a, "kzg_set_pairs", false, n == 0 || (lhs_out_aff && z2_out_aff) ? (const void*)ctx : nullptr, "lhs_out_aff or z2_out_aff"));
  if (n == 0) return KEAKI_OK;
  const SetHostIn in(a);
  ST_TRY(in.reserve(ctx));
  ST_TRY(reserve(ctx, ctx->sp_pairs, n * (G1_AFF_BYTES + G2_AFF_BYTES)));
  ItemStager items{ctx, com_aff, com_stride, nullptr, nullptr, 0, nullptr, nullptr, n};      // one commitment: in io_e
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);
  ST_TRY(in.put(ctx, feed, items, a));
  char* out = (char*)ctx->sp_pairs.p;
  ST_TRY(set_pairs_core(ctx, srs_g1, srs_g2, a, out, out + n * G1_AFF_BYTES));
  prefault_out(ctx, z2_out_aff, n * G2_AFF_BYTES);
  HIP_TRY(ctx, hipMemcpyAsync(lhs_out_aff, out, n * G1_AFF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, z2_out_aff, out + n * G1_AFF_BYTES, n * G2_AFF_BYTES);
}

keaki_status keaki_hip_kzg_verify_sets_each_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const void* d_com_aff,
                                                int32_t com_stride, const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values,
                                                size_t item_stride, size_t k, const void* d_proofs_aff, size_t n, void* d_status, uint64_t* n_bad,
                                                uint64_t* first_bad, void* d_lhs_out_aff, void* d_z2_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_sets_each");
  const VsArgs a = {srs_g1, srs_g2, d_com_aff, d_points, d_values, d_proofs_aff, nullptr, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(set_pairs_args(ctx, a, "kzg_verify_sets_each", true, n_bad && (n == 0 || d_status) ? (const void*)n_bad : nullptr, "n_bad or status"));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  SeWork w;
  ST_TRY(set_each_reserve(ctx, n, false, &w));
  return set_each_core(ctx, srs_g1, srs_g2, a, w, d_lhs_out_aff ? d_lhs_out_aff : w.a, d_z2_out_aff ? d_z2_out_aff : w.z2, d_status, n_bad, first_bad);
}

keaki_status keaki_hip_kzg_verify_sets_each(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                            int32_t com_stride, const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values,
                                            size_t item_stride, size_t k, const uint64_t* proofs_aff, size_t n, uint8_t* status, uint64_t* n_bad,
                                            uint64_t* first_bad, uint64_t* lhs_out_aff, uint64_t* z2_out_aff) {
  CTX_GUARD(ctx);                 // held across upload -> kernels -> download: the io buffers belong to this call until it returns
  TRACE_SCOPE("keaki.kzg_verify_sets_each");
  VsArgs a = {srs_g1, srs_g2, com_aff, points, values, proofs_aff, nullptr, omega, com_stride, point_mode, item_stride, k, n};
  ST_TRY(set_pairs_args(ctx, a, "kzg_verify_sets_each", true, n_bad && (n == 0 || status) ? (const void*)n_bad : nullptr, "n_bad or status"));
  if (n == 0) { verify_each_empty(n_bad, first_bad); return KEAKI_OK; }
  const SetHostIn in(a);
  SeWork w;
  ST_TRY(set_each_reserve(ctx, n, true, &w));
  ST_TRY(in.reserve(ctx));
  ItemStager items{ctx, com_aff, com_stride, nullptr, nullptr, 0, nullptr, proofs_aff, n};      // one commitment: in io_e
  ST_TRY(items.reserve());
  CopyFeed feed(ctx);
  ST_TRY(in.put(ctx, feed, items, a));
  ST_TRY(set_each_core(ctx, srs_g1, srs_g2, a, w, w.a, w.z2, w.status, n_bad, first_bad));
  if (lhs_out_aff) HIP_TRY(ctx, hipMemcpyAsync(lhs_out_aff, w.a, n * G1_AFF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (z2_out_aff) HIP_TRY(ctx, hipMemcpyAsync(z2_out_aff, w.z2, n * G2_AFF_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, status, w.status, n);
}
