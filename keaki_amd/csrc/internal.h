// Internal (not installed) declarations shared by the translation units of libkeaki_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/keaki_hip.h"

namespace keaki_internal {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
// Widest forced windows. A plan with more than 2^22 buckets to sort (generic: the buckets of all windows; window tables: those of the largest
// window) is beyond the two-pass bucket sort (msm.hip.h: part_make_shape, 2^11 bins of 2^11 buckets): generic 20 .. 24 and shared 24 bits
// could never run. msm_g2.hip checks both limits against the plans. keaki_hip_ctx_set_option refuses the widths between a limit and 24,
// tune_from_env ignores them; any other value outside 3 .. 24 means automatic, as it always did.
constexpr int MSM_C_MAX = 19, MSM_C_SHARED_MAX = 23;
// vec_update (vec_update.hip): entries of the change list a pass of the proof kernel takes (8 scalar words per entry and lane in LDS: 16 KB a wave)
constexpr uint32_t UPD_K_PASS = 8;
// kzg verify_cosets (kzg_cosets.hip): Fr elements of one LDS tile (VC_TILE_ELEMS / l items) | most workgroups of the transform kernel (= partial rows the finish kernel folds)
constexpr uint32_t VC_TILE_ELEMS = 1024, VC_MAX_BLOCKS = 1024;
// kzg verify_sets (kzg_sets.hip): most workgroups of the polynomial kernel (= partial rows the finish kernel folds)
constexpr uint32_t VS_MAX_BLOCKS = 1024;
inline bool msm_c_too_wide(long long v, int max) { return v > max && v <= 24; }
// Tuning / diagnostic switches of a context: every member but alloc_limit is an option of keaki_hip_ctx_set_option by its own name, with an
// entry in TUNE_OPTIONS (api.hip). The environment is read ONCE, in keaki_hip_ctx_create (tune_from_env); afterwards only
// keaki_hip_ctx_set_option changes them (under the context lock). No other code in the library calls getenv.
struct Tuning {
  int msm_c = 0;                 // KEAKI_MSM_C / "msm_c": window bits of the generic MSM, 3 .. MSM_C_MAX; 0 (or any value outside 3 .. 24) = choose_window
  int msm_c_shared = 0;          // KEAKI_MSM_C_SHARED / "msm_c_shared": window target of the SRS window tables, 3 .. MSM_C_SHARED_MAX; 0 (or outside 3 .. 24) = choose_window_shared
  int msm_short_tables = -1;     // KEAKI_MSM_SHORT_TABLES / "msm_short_tables": an MSM over less than half of an SRS with window tables uses them (1, and automatic = -1) or the generic path (0)
  int reduce_l = 0;              // KEAKI_REDUCE_L / "reduce_l": chunk length of the bucket reduction, 0 = automatic
  int part_shift = -1;           // KEAKI_PART_SHIFT / "part_shift": log2 of the bucket sort's bin count, -1 = automatic
  bool acc_u29 = true;           // KEAKI_ACC_U29 / "acc_u29": G1 bucket kernel in the 29-bit lazy limbs (A/B switch for profiling)
  bool acc_u29_g2 = true;        // KEAKI_ACC_U29_G2 / "acc_u29_g2"
  bool acc_prefetch = true;      // KEAKI_ACC_PREFETCH / "acc_prefetch": the G1 bucket kernel requests the next pair's table row an iteration ahead (A/B switch)
  bool acc_idxq = true;          // KEAKI_ACC_IDXQ / "acc_idxq": the G1 bucket kernel reads its index stream by aligned 64-byte groups through a lane-private LDS slot (0: one 4-byte load per entry, as until round 5; A/B switch)
                                 // acc_nt, acc_prefetch and acc_idxq choose among the WHOLE-MSM kernels only: the passes of a chunked call always run the default kernel
  bool cs_masked = true;         // KEAKI_CS_MASKED / "cs_masked": pass 2 of the bucket sort skips empty gather slots under the exec mask (0: every empty slot counts into a dummy word per lane, as in round 4; A/B switch: 0.84 -> 0.70 ms at 2^24)
  bool acc_nt = false;           // KEAKI_ACC_NT / "acc_nt": non-temporal loads of the table rows in the G1 bucket kernel
  bool fk_uniform = true;        // KEAKI_FK_UNIFORM / "fk_uniform": sliding-window ladder in the wave-uniform FK23 stages
  bool fk_gtab = true;           // KEAKI_FK_GTAB / "fk_gtab": window tables of the per-lane-scalar ladders in a lane-contiguous workspace (0: private memory)
  bool fk_radix4 = true;        // KEAKI_FK_RADIX4 / "fk_radix4": two wave-uniform stages in one radix-4 pass (three doubling chains instead of four)
  bool fk_addsub29 = true;      // KEAKI_FK_ADDSUB29 / "fk_addsub29": the butterflies' add + subtract in the lazy limbs, shared products once (A/B switch)
  bool fb_occ1 = false;          // KEAKI_FB_OCC1 / "fb_occ1": one wave per SIMD for the G2 fixed-base kernel at any batch size
  int pair_wide_max = -1;        // KEAKI_PAIR_WIDE_MAX / "pair_wide_max": pairing batches up to this size run the twelve-lanes-per-pairing kernel; -1 = automatic, 0 = never
  bool pair_two_waves = true;    // KEAKI_PAIR_TWO_WAVES / "pair_two_waves": up to 1,024 pairings with lines on the fly run the line functions on a second wave (A/B switch)
  int gt_wb_b = 0;               // KEAKI_GT_WB_B / "gt_wb_b": window bits of the table of e(g1, g2), 0 = automatic (20 / 16)
  long long encap_multi_single_min = 16384;   // KEAKI_ENCAP_MULTI_SINGLE_MIN / "encap_multi_single_min": a group of encap_multi / encrypt_multi with at least this many items runs the single-commitment path (GT tables), smaller groups the fused per-item pairing; 0 = never the single path (measured: the smallest k of 1,024 / 4,096 / 16,384 / 65,536 at which the single route wins, profiles/encap_multi_times.txt; the estimate before the sweep was 8,192)
  long long encap_gt = -1;       // KEAKI_ENCAP_GT / "encap_gt": batch size from which encap takes the GT fixed-base path; -1 = automatic (always, since round 4)
  bool host_prefault = true;     // KEAKI_HOST_PREFAULT / "host_prefault": first-touch (write zeros into) and madvise(MADV_HUGEPAGE) the caller's OUTPUT arrays while the kernels run, on helper threads for chunked batches; 0 = the library never touches caller memory except through the device copies
  bool pipe_chunks = true;       // KEAKI_PIPE_CHUNKS / "pipe_chunks": host-pointer batches (KEM, MSM) run as chunk pipelines over a copy stream; 0 = upload, kernels, download in that order on the context's stream
  int msm_pipe_chunks = -1;      // KEAKI_MSM_PIPE_CHUNKS / "msm_pipe_chunks": chunks of a host-pointer MSM (upload under the kernels); -1 = automatic, 0 / 1 = one copy in front, k = k chunks at any length
  long long msm_pipe_min = 1 << 20;   // KEAKI_MSM_PIPE_MIN / "msm_pipe_min": automatic chunking from this many scalars on
  int msm_pipe_growth = 160;     // KEAKI_MSM_PIPE_GROWTH / "msm_pipe_growth": size of chunk j + 1 in percent of chunk j (100 = equal chunks; round 6: 160, measured best or tied at 2^20 .. 2^24, profiles/r06_msm_pipe_growth.txt; 140 until round 5)
  int fk_coset_group = 0;        // KEAKI_FK_COSET_GROUP / "fk_coset_group": terms per Straus group of the FK23 coset openings' pointwise kernel, 1, 2 or 4; 0 = FKC_G (fk_coset_plan.h); 1 = one ladder per term (A/B switch)
  long long fk_coset_min_lanes = 0;   // KEAKI_FK_COSET_MIN_LANES / "fk_coset_min_lanes": the pointwise launch of the FK23 coset openings splits a position's terms over lanes while it has fewer lanes than this; 0 = FKC_SPLIT_MIN_LANES
  int verify_cosets_blocks = 0;  // KEAKI_VERIFY_COSETS_BLOCKS / "verify_cosets_blocks": workgroups of verify_cosets' transform kernel, 1 .. VC_MAX_BLOCKS; 0 = automatic (three per compute unit, what its LDS holds; a test sets 2 to make a workgroup run several tiles)
  int verify_sets_blocks = 0;    // KEAKI_VERIFY_SETS_BLOCKS / "verify_sets_blocks": workgroups of verify_sets' polynomial kernel, 1 .. VS_MAX_BLOCKS; 0 = automatic (three per compute unit, what its registers allow; a test sets 1 or 2 to make a workgroup run several tiles)
  long long coset_rows_min_lanes = 0;   // KEAKI_COSET_ROWS_MIN_LANES / "coset_rows_min_lanes": the row kernel of kzg coset_pairs splits an item's l bases over lanes while a launch has fewer lanes than this; 0 = CR_MIN_LANES (coset_rows_plan.h)
  int coset_rows_route = 0;      // KEAKI_COSET_ROWS_ROUTE / "coset_rows_route": how kzg coset_pairs sums its rows: 1 = the handle's window table over the first l SRS points, 2 = the batched MSM; 0 = by plan (coset_rows_plan.h: cr_route)
  int coset_rows_wb = 0;         // KEAKI_COSET_ROWS_WB / "coset_rows_wb": window bits of that table, 8, 10 or 13; 0 = by plan (coset_rows_plan.h: cr_wb; the switch of the width sweep)
  int set_rows_wb = 0;           // KEAKI_SET_ROWS_WB / "set_rows_wb": window bits of the G2 handle's table of kzg set_pairs, 8, 10 or 13; 0 = by plan (set_rows_plan.h: sr_wb; the switch of the width sweep)
  long long set_rows_min_lanes = 0;     // KEAKI_SET_ROWS_MIN_LANES / "set_rows_min_lanes": the G2 row kernel of kzg set_pairs splits an item's k bases over lanes while a launch has fewer lanes than this; 0 = SR_MIN_LANES (set_rows_plan.h)
  int set_each_route = 0;        // KEAKI_SET_EACH_ROUTE / "set_each_route": how kzg verify_sets_each decides its items: 1 = the fused kernel k_pairing2v, 2 = two Miller loops per item, a pairwise GT product, the final exponentiation and a comparison with one; 0 = by plan (set_rows_plan.h: se_route, which is route 2 at every n, as measured)
  int vec_update_k_pass = 0;     // KEAKI_VEC_UPDATE_K_PASS / "vec_update_k_pass": entries of the change list per pass of vec_update's proof kernel, 1 .. UPD_K_PASS; 0 = UPD_K_PASS
#ifdef KEAKI_DIAG
  unsigned diag_row_mask = 0;    // "diag_row_mask" (ONLY in the diagnostic build, `make -C keaki_amd/csrc diag`; never in libkeaki_hip.so): the table-row index of every (row, sign) entry of the bucket-ordered stream is ANDed with this mask before the bucket kernel runs, so its gathers hit a table of (mask + 1) x 64 B -- the arithmetic, the instruction stream and the kernel binary stay the shipped ones, the RESULT IS WRONG by construction (bench_tools/r6_bucket_clock_diag.py)
#endif
  size_t alloc_limit = 0;        // keaki_hip_debug_set_alloc_limit: single allocations above it fail with KEAKI_ERR_OOM; 0 = none
};
// A device table that belongs to ONE point, its key (the W affine words of the point): the window tables of [tau]_2 and the GT table of a
// commitment. A rebuild runs invalidate() -> launches -> publish(), so a build that failed half way is never taken for valid.
template <int W>
struct KeyedTable {
  DevBuf buf;
  bool valid = false;
  uint32_t wb = 0;                        // window bits of the table in buf
  uint64_t key[W] = {};
  bool holds(const uint64_t* k) const { return valid && memcmp(k, key, sizeof(key)) == 0; }
  void invalidate() { valid = false; }
  void publish(const uint64_t* k, uint32_t bits) { memcpy(key, k, sizeof(key)); wb = bits; valid = true; }
};
// The cache of encapsulate and kzg verify (api.hip: the KEM composites; api_kzg.hip: keaki_hip_kzg_verify). A table built once per context stands beside its
// ready bit, which is set only after EVERY step of the build succeeded; the tables of one point are KeyedTables.
struct KemState {
  // 16-bit window tables for batches of >= 256 items: of the generators (with room for the 13-bit table that the per-item-pairing path rebuilds for
  // each batch's commitment) and of [tau]_2 | small (8-bit) tables for smaller batches and kzg verify: of g2 and [tau]_2 | of g1 (verify only)
  DevBuf fb_g1_gen, fb_g2_gen, fb_com, fbs_g2_gen, fbs_g1_gen;
  bool fb_ready = false, fbs_ready = false, fbs_g1_ready = false, verify_tables_ready = false;
  KeyedTable<16> fb_tau, fbs_tau;
  // kzg verify's small in/out block | line sequence of g2 | line tables and points of 2^s g2, s < 320 (api.hip: g2pow_tables)
  DevBuf verify_io, g2gen_lines, g2pow_lines, g2pow_pts;
  bool verify_ready = false, g2gen_lines_ready = false, g2pow_ready = false;
  // GT tables: B = e(g1, g2) once per context at gt_b_wb bits, A = e(C, g2) per commitment; gt_base holds the powers of the LAST table built
  DevBuf gt_base, gt_tab_b;
  bool gt_b_ready = false, gt_b_fallback = false;   // fallback: the wide table of B did not fit once, stay at 16 bits
  uint32_t gt_b_wb = 0;
  KeyedTable<8> gt_a;
  bool gt_a_pending_aux = false;          // the A-table build on aux.stream has not been waited for by `stream` yet (api.hip: wait_aux)
  KeyedTable<16> tau_lines;               // kzg verify_each: line sequence of the last [tau]_2 (rebuilt when another one arrives)
  uint64_t seen_com[8] = {};              // commitment of the last encap call and how many consecutive calls carried it
  uint32_t seen_com_runs = 0;
  // every DevBuf above with its memory class (keaki_hip_ctx_memory: 1 = workspace, 2 = GT / fixed-base tables): a new table is added HERE
  template <class F> void for_each_buf(F&& f) {
    for (DevBuf* b : {&g2gen_lines, &g2pow_lines, &g2pow_pts, &verify_io, &tau_lines.buf}) f(b, 1);
    for (DevBuf* b : {&fb_g1_gen, &fb_g2_gen, &fb_com, &fb_tau.buf, &fbs_g2_gen, &fbs_tau.buf, &fbs_g1_gen, &gt_a.buf, &gt_tab_b, &gt_base}) f(b, 2);
  }
};
keaki_status fail(keaki_hip_ctx* ctx, keaki_status code, const char* fmt, ...);
#define HIP_TRY(ctx, call)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return keaki_internal::fail(ctx, e_ == hipErrorOutOfMemory ? KEAKI_ERR_OOM : KEAKI_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                           \
  } while (0)
#define ST_TRY(call)                 \
  do {                               \
    keaki_status s_ = (call);        \
    if (s_ != KEAKI_OK) return s_;   \
  } while (0)

// A side stream of a context with its events, created on first use and released with the context (the stream LAST: it says that all exist).
inline keaki_status lane_ready(keaki_hip_ctx* ctx, hipStream_t& s, std::initializer_list<hipEvent_t*> evs) {
  if (s) return KEAKI_OK;
  for (hipEvent_t* e : evs) if (!*e) HIP_TRY(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
  HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return KEAKI_OK;
}
inline void lane_destroy(hipStream_t& s, std::initializer_list<hipEvent_t*> evs) {
  for (hipEvent_t* e : evs) if (*e) (void)hipEventDestroy(*e);
  if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
}
// host-pointer calls in chunks (api_host.h: CopyFeed; api.hip: pipelined): uploads and downloads of the neighbouring chunks on a stream of their own.
// [in: chunk staged | done: chunk computed], one pair per buffer half
struct HostPipe {
  hipStream_t copy_stream = nullptr;
  hipEvent_t in[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  keaki_status ready(keaki_hip_ctx* ctx) { return lane_ready(ctx, copy_stream, {&in[0], &in[1], &done[0], &done[1]}); }
  void destroy() { lane_destroy(copy_stream, {&in[0], &in[1], &done[0], &done[1]}); }
};
// latency-bound side jobs: the GT table of a new commitment (api.hip: a_table) with ev = [go | done], and the quotients of a chunked
// kzg_open (api.hip: open_chunked) with open_ev = [chunk's quotient ready x 2 | start]
struct AuxLane {
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr}, open_ev[3] = {nullptr, nullptr, nullptr};
  keaki_status ready(keaki_hip_ctx* ctx) { return lane_ready(ctx, stream, {&ev[0], &ev[1], &open_ev[0], &open_ev[1], &open_ev[2]}); }
  void destroy() { lane_destroy(stream, {&ev[0], &ev[1], &open_ev[0], &open_ev[1], &open_ev[2]}); }
};
}  // namespace keaki_internal

struct keaki_hip_ctx {
  int device = 0;
  uint32_t n_cu = 256;           // compute units of the device (grid size of the persistent kernels)
  keaki_internal::Tuning tune;
  // bytes this context allocated and still holds, by class (keaki_hip_ctx_memory): SRS window tables + FK23 transforms of handles built
  // through it | grow-only workspaces | GT / fixed-base tables of encapsulate
  std::atomic<size_t> mem_tables{0};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::recursive_mutex mu;   // recursive: host-pointer entry points hold it across stage -> *_dev -> download
  std::string err;
  // grow-only workspaces (all used in stream order); fb_bases: scratch of g1/g2_fb_table_run
  keaki_internal::DevBuf digits, hist, offsets, cursor, sorted, buckets, acc29, partials, wsums, tmp_a, tmp_b, tmp_c, io_a, io_b, io_c, io_d, io_e, perm, heavy, fb_bases;
  keaki_internal::KemState kem;                     // every cached table of encapsulate and kzg verify
  keaki_internal::DevBuf pair_ws;                   // per-item slots of the final exponentiation (pairing.hip.h)
  keaki_internal::DevBuf fk_tab;                    // window tables of the per-lane-scalar ladders of FK23: 1 KB per lane of a launch (64 x 16 B), at most 2 GB (fft_g1.hip)
  keaki_internal::DevBuf mb_canon, mb_wsums, mb_q;  // batched MSM / open (msm_batch.hip): biased canonical scalars of a pass (32 B each) | window sums (128 B per row and window) | quotient rows of open_batch
  keaki_internal::DevBuf fkb_pts, fkb_fr;           // batched FK23 (fk_batch.hip): the 2d x M Jacobian points of a pass, position-major | its scalar rows (96 B per coefficient) and the call's twiddle tables
  keaki_internal::DevBuf em_offsets;                // encap_multi / encrypt_multi, _dev forms: the device copy of the caller's group offsets (8 B per group)
  keaki_internal::DevBuf vb_io, vb_s;               // kzg verify_batch: the small in/out block with the reduction's partials | the scalars gamma_i z_i of the second MSM (32 B per item)
  keaki_internal::DevBuf ve_io, ve_pts, ve_out;     // kzg verify_each: the small in/out block (counters, commitment, [tau]_2, omega) | L and -proof of a launch chunk (128 B per item) | host form: the status bytes and L of the whole call
  keaki_internal::DevBuf vu_io, vu_work, vu_pass;   // vec_update: host form: indices, deltas, commitment and proofs of the call | the 2d Jacobian points of a table build, the terms of the commitment | header and window tables of a pass
  keaki_internal::DevBuf ks_io, ks_q;               // KZG set openings: points, values, Z, weights, I and the small results of a call | the quotient and the work of its passes (kzg_multi.hip)
  keaki_internal::DevBuf vc_io, vc_work;            // kzg verify_cosets: the small in/out block (VcLayout, api_kzg.hip) | s, 1 / h, -J, g and the partial rows of a call (kzg_cosets.hip: verify_cosets_layout)
  keaki_internal::DevBuf cp_work, cp_pairs, cp_in;  // kzg coset_pairs: 1 / h (n Fr), then the rows, the XYZZ sums and (route 2) the Jacobian sums of a launch chunk | verify_cosets_each: A, c and the zero values of the call; host forms: + the outputs | host forms: the values
  keaki_internal::DevBuf vs_io, vs_work;            // kzg verify_sets: the small in/out block (VsLayout, api_kzg.hip) | the scalar rows, the weights, -J, g, the partial rows and (point_mode 1) the derived points of a call (kzg_sets.hip: verify_sets_layout)
  keaki_internal::DevBuf sp_work, sp_pairs, sp_in;  // kzg set_pairs: weights, derived points, the two scalar rows, the XYZZ sums and (G1 route 2) the Jacobian sums of a launch chunk | verify_sets_each: A, Z2 and the pairing side's blocks of a launch chunk; host forms: + the outputs | host forms: points and values
  keaki_internal::DevBuf gp_work;                   // pairing_product: the Miller-loop outputs of a call (384 B per pair), the partial products and the product
  keaki_internal::DevBuf fc_work;                   // FK23 coset openings (fk_coset.hip): twiddles, hat_a, the partial sums and the two transforms of a call; host forms: + coefficients and proofs
  // every DevBuf above with its memory class, kem's included (KemState::for_each_buf): what keaki_hip_ctx_destroy and _trim free and
  // keaki_hip_ctx_memory counts. A new workspace is added HERE.
  template <class F> void for_each_buf(F&& f) {
    for_each_scratch(f);
    kem.for_each_buf(f);
  }
  // the DevBufs declared directly above: scratch, every word a call reads was written by a kernel or copy of the SAME call, so
  // keaki_hip_debug_poison_workspaces may overwrite all of them between calls. kem's buffers are caches behind ready / valid bits and are not in this list.
  template <class F> void for_each_scratch(F&& f) {
    f(&fb_bases, 2);
    for (keaki_internal::DevBuf* b : {&digits, &hist, &offsets, &cursor, &sorted, &buckets, &acc29, &partials, &wsums, &tmp_a, &tmp_b, &tmp_c, &io_a, &io_b, &io_c,
                                      &io_d, &io_e, &perm, &heavy, &pair_ws, &fk_tab, &mb_canon, &mb_wsums, &mb_q, &fkb_pts, &fkb_fr, &em_offsets, &vb_io, &vb_s,
                                      &ve_io, &ve_pts, &ve_out, &vu_io, &vu_work, &vu_pass, &ks_io, &ks_q, &fc_work, &vc_io, &vc_work, &cp_work, &cp_pairs, &cp_in, &vs_io, &vs_work, &sp_work, &sp_pairs, &sp_in, &gp_work})
      f(b, 1);
  }
  int poison_new = -1;           // keaki_hip_debug_poison_workspaces(.., also_new = 1): dev_alloc fills every new allocation with this byte; -1 = off
  // instrumentation
  bool timing = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_bucket_ms = -1.f, last_total_ms = -1.f;
  int last_c = 0;
  bool timing_pending = false;
  // FK23 openings: [start | after the 2d pointwise products | after the two size-d group transforms | after the affine conversion]
  hipEvent_t fk_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool fk_timing_pending = false;
  float last_fk_ms[3] = {-1.f, -1.f, -1.f};      // pointwise products, butterfly stages (k_g1_fft_stage_map), whole device pipeline
  keaki_internal::HostPipe pipe;                    // the copy stream of the chunked host-pointer calls
  keaki_internal::AuxLane aux;                      // the stream of the latency-bound side jobs
};

namespace keaki_internal {

// Makes `device` the calling thread's current HIP device for the scope and puts the caller's own choice back on exit: a host application
// (PyTorch, another HIP library) that shares the thread never sees its current device change behind its back.
struct DeviceScope {
  int prev = -1;
  bool ok = true;
  explicit DeviceScope(int device) {
    if (device < 0) return;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return;
    ok = hipSetDevice(device) == hipSuccess;
    if (ok) prev = cur;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

keaki_status reserve(keaki_hip_ctx* ctx, DevBuf& b, size_t bytes);
// hipMalloc behind the library's one allocation gate. keaki_hip_debug_set_alloc_limit(ctx, bytes) makes every single allocation of this
// context above that size fail with KEAKI_ERR_OOM, which is how the tests exercise the optional-memory fallbacks (SRS window tables,
// the wide GT table) and a refused rebuild of a handle's FK23 transform. One allocation stays outside on purpose: the points of
// keaki_hip_srs_g*_upload (api.hip: srs_upload), which tests upload while a limit is set.
keaki_status dev_alloc(keaki_hip_ctx* ctx, void** p, size_t bytes);
keaki_status launch_check(keaki_hip_ctx* ctx, const char* what);
inline uint32_t cdiv(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

// Chunked form of one MSM (the host-pointer entries, api.hip): the (scalar, point) pairs are cut into point-range chunks; every chunk
// runs its own tile sort -> chunk sort -> size order -> bucket pass, the bucket pass going on from what the earlier chunks left in the
// buckets (msm.hip.h: Acc29 / `cont`), and ONE reduction tail closes the call. `stage(j)` is called right before the kernels of chunk j
// are enqueued: the caller uploads that chunk's scalars there (on its copy stream) and makes the context's stream wait for them, so the
// upload of chunk j + 1 runs under the kernels of chunk j. The sum is the same group element whatever the cut (exact arithmetic).
struct MsmPipe {
  std::vector<std::pair<size_t, size_t>> ranges;     // chunk j = pairs [first, first + second); the ranges partition [0, n), in ANY order
  std::function<keaki_status(size_t)> stage;         // (the quotient of `open` is produced from the top coefficient down: its chunks come last-first)
};

// launchers implemented in the kernel translation units (all enqueue on ctx->stream, no sync)
keaki_status msm_g1_run(keaki_hip_ctx* ctx, const void* d_points, size_t srs_len, const void* d_scalars, size_t n, void* d_out_jac,
                        const void* d_table = nullptr, int c_table = 0, const MsmPipe* pipe = nullptr);
keaki_status msm_g1_precompute_run(keaki_hip_ctx* ctx, const void* d_points, size_t N, int* c_table_out, size_t* table_bytes_out, void** d_table_out);
keaki_status msm_g2_run(keaki_hip_ctx* ctx, const void* d_points, size_t srs_len, const void* d_scalars, size_t n, void* d_out_jac,
                        const void* d_table = nullptr, int c_table = 0, const MsmPipe* pipe = nullptr);
keaki_status msm_g2_precompute_run(keaki_hip_ctx* ctx, const void* d_points, size_t N, int* c_table_out, size_t* table_bytes_out, void** d_table_out);
keaki_status g1_sum_run(keaki_hip_ctx* ctx, const void* d_points_jac, size_t k, void* d_out_jac);
keaki_status g1_mul_batch_run(keaki_hip_ctx* ctx, const void* d_pts, int stride, const void* d_scalars, size_t n, void* d_out);
keaki_status g2_mul_batch_run(keaki_hip_ctx* ctx, const void* d_pts, int stride, const void* d_scalars, size_t n, void* d_out);
keaki_status encap_g1_run(keaki_hip_ctx* ctx, const void* d_com, const void* d_values, const void* d_r, size_t n, void* d_out);
size_t pairing_launch_items();      // items per k_pairing launch (the slots of the final exponentiation bound it)
keaki_status pairing_run(keaki_hip_ctx* ctx, const void* d_g1, const void* d_g2, int g2_stride, size_t n, void* d_gt, const void* d_fixed_lines = nullptr,
                         uint32_t lines_stride = 0);
uint32_t g2_prepared_lines();                 // Line entries of one table
// kzg verify: A = com - value g1, Q = [tau]_2 - point g2 from the wb-bit window tables of the generators (sixteen lanes per sum)
keaki_status verify_points_run(keaki_hip_ctx* ctx, const void* d_tab_g1, const void* d_tab_g2, uint32_t wb, const void* d_com, const void* d_tau_g2,
                               const void* d_value, const void* d_point, void* d_out_a, void* d_out_q);
size_t g2_prepared_bytes();
// out[i] = e(P_(i * p_stride), Q_i) as 12 Fq in the 2^261 form, Q_i given by its line table d_lines + i * lines_stride lines
keaki_status pairing_raw_fixed_run(keaki_hip_ctx* ctx, const void* d_g1, uint32_t p_stride, size_t n, const void* d_lines, uint32_t lines_stride, void* d_out);
size_t gt_table_bytes(uint32_t wb);
uint32_t gt_table_powers(uint32_t wb);      // powers of two a table needs: wb * windows
keaki_status gt_table_run(keaki_hip_ctx* ctx, const void* d_pows, void* d_table, uint32_t wb);   // d_pows: base^(2^s), 12 Fq each
// gt[i] = serialize(acc_in[i] (or one) * A^(r_i) (tab_a given) * B^(-beta_i r_i) (tab_b given)); acc_out given: the product stays raw (12 Fq per item)
keaki_status gt_encap_exp_run(keaki_hip_ctx* ctx, const void* d_tab_a, uint32_t wb_a, const void* d_tab_b, uint32_t wb_b, const void* d_betas,
                              const void* d_rs, size_t n, void* d_gt, const void* d_acc_in = nullptr, void* d_acc_out = nullptr);
keaki_status miller_only_run(keaki_hip_ctx* ctx, const void* d_g1, const void* d_g2, size_t n, void* d_out);
keaki_status final_exp_only_run(keaki_hip_ctx* ctx, const void* d_in, size_t n, void* d_gt);
keaki_status g2_prepare_run(keaki_hip_ctx* ctx, const void* d_q, void* d_lines, uint32_t n_points = 1);   // line sequence of a fixed Q (2^261 form: internal)
keaki_status lines_to256_run(keaki_hip_ctx* ctx, const void* d_lines261, void* d_lines256);   // the same table in the ABI's 2^256 form (test hook)
keaki_status blake3_gt_run(keaki_hip_ctx* ctx, const void* d_gt, size_t n, void* d_key, size_t msg_len, bool xor_into = false);   // xor_into: key ^= in place (the DEM)
keaki_status g2_generator_to(keaki_hip_ctx* ctx, void* d_dst);  // writes the affine G2 generator (128 B)
keaki_status g1_generator_to(keaki_hip_ctx* ctx, void* d_dst);  // affine G1 generator (64 B)
size_t fb_table_entries(uint32_t wb);                                                          // window-table entries per base at window width wb
keaki_status g1_fb_table_run(keaki_hip_ctx* ctx, const void* d_base, void* d_table, uint32_t wb);    // table[j * entries + d] = d 2^(wb j) base
keaki_status g1_fb_tables_run(keaki_hip_ctx* ctx, const void* d_bases, uint32_t n_bases, void* d_table, uint32_t wb);   // table[(b windows + j) entries + d] = d 2^(wb j) bases[b]
keaki_status g2_fb_table_run(keaki_hip_ctx* ctx, const void* d_base, void* d_table, uint32_t wb);
keaki_status g2_pow2_multiples_run(keaki_hip_ctx* ctx, const void* d_base, uint32_t count, void* d_out);   // out[s] = 2^s base (affine), lane s doubles s times
keaki_status encap_g1_fixed_run(keaki_hip_ctx* ctx, const void* d_tab_a, uint32_t wb_a, const void* d_tab_b, uint32_t wb_b, const void* d_xs, const void* d_rs, size_t n, void* d_out);
keaki_status encap_g2_fixed_run(keaki_hip_ctx* ctx, const void* d_tab_a, uint32_t wb_a, const void* d_tab_b, uint32_t wb_b, const void* d_xs, const void* d_rs, size_t n, void* d_out, bool share_simds = false);
// encap_multi, G1 side (kem_multi.hip): out[i] = r_i (C_j - beta_i g1) for item first + i of group j, offsets[j] <= first + i < offsets[j + 1];
// d_offsets: m + 1 u64 (device), d_tab_g1: the wb-bit window table of g1; n < 2^31
keaki_status encap_multi_g1_run(keaki_hip_ctx* ctx, const void* d_coms, const void* d_offsets, size_t m, uint64_t first, const void* d_tab_g1, uint32_t wb,
                                const void* d_values, const void* d_r, size_t n, void* d_out);
keaki_status g1_curve_check_run(keaki_hip_ctx* ctx, const void* d_pts, size_t n, void* d_bad2);   // d_bad2: u64 count, u64 first index
keaki_status g2_curve_check_run(keaki_hip_ctx* ctx, const void* d_pts, size_t n, void* d_bad2);
// top_is_carry: d_c[n - 1] is not a coefficient but the suffix value carried in from the chunk above (its quotient slot is left alone)
keaki_status open_quotient_run(keaki_hip_ctx* ctx, const void* d_c, size_t n, const uint64_t* z, void* d_q, void* d_value, void* d_work, bool top_is_carry = false);
size_t open_quotient_work_bytes(size_t n);           // size of d_work for n coefficients
keaki_status fr_fft_run(keaki_hip_ctx* ctx, void* d_data, uint32_t log2n, const uint64_t* omega, const uint64_t* scale_or_null, void* d_tw);
void fr_powers_run(keaki_hip_ctx* ctx, const uint64_t* omega, uint32_t n, void* d_out);      // d_out[k] = omega^k, k < n
// FK23 from the coefficients (api.hip: open_fk_from_poly): the scalar half fills d_fr_work and says where hat_a and the twiddles of
// fk_hat_s_run / open_fk_run lie in it. Workspace sizes of the scalars and of open_fk_run's 2d Jacobian points:
size_t open_fk_poly_fr_bytes(uint32_t log2d);
size_t open_fk_poly_g_bytes(uint32_t log2d);
struct FkPolyScalars { const void *hat_a, *tw, *twi; };
keaki_status open_fk_poly_scalars_run(keaki_hip_ctx* ctx, uint32_t log2d, const void* d_p, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                                      const uint64_t* inv_2d, void* d_fr_work, FkPolyScalars* out);
keaki_status fk_hat_s_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2d, const void* d_tw2d, void* d_hat_s);
keaki_status open_fk_run(keaki_hip_ctx* ctx, const void* d_hat_s, uint32_t log2d, const void* d_hat_a, const void* d_tw2d, const void* d_tw2d_inv,
                         void* d_work, void* d_proofs_aff);
// FK23 sharded over 2^rho ranks (fft_g1.hip): this rank's plan and device buffers (owned by the api layer)
struct FkShard {
  uint32_t log2d = 0, rho = 0, rank = 0;
  uint64_t omega[4], omega_inv[4], inv_2d[4];
  void *tw = nullptr, *twi = nullptr;     // omega_2d^k, omega_2d^-k, k < d
  void *hat_a = nullptr, *coeffs = nullptr;   // 2d Fr, d Fr
  void *hat_s = nullptr, *work = nullptr;     // 2d / R Jacobian points each
  void *e = nullptr;                          // d / R Jacobian points: the even half of the products, from step 0 to step 2
  bool tables_ready = false, hat_s_ready = false;
};
keaki_status fk_shard_setup_run(keaki_hip_ctx* ctx, FkShard& fk, const void* d_srs, int step, void* d_send, void* d_recv);
keaki_status fk_shard_open_run(keaki_hip_ctx* ctx, FkShard& fk, int step, void* d_send, void* d_recv, void* d_out_aff);
// kzg verify_batch (kzg_batch.hip): d_s_out[i] = gamma_i z_i (point_mode 0: z_i = d_points[i]; 1: z_i = d_points[0]^i) and d_gt_out = (g, -t) =
// (sum gamma_i, -sum gamma_i y_i), through d_partials (verify_batch_partials_bytes()); 1 <= n < 2^31
constexpr uint32_t VB_MAX_BLOCKS = 1024;
size_t verify_batch_partials_bytes();
keaki_status verify_batch_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const void* d_values, size_t n,
                                      void* d_s_out, void* d_partials, void* d_gt_out);
// kzg verify_cosets (kzg_cosets.hip), n items of l = 2^log2l values each, 1 <= n, n * l < 2^31, l <= KEAKI_SET_MAX. The workspace of a call
// (verify_cosets_work_bytes) holds s_k = gamma_k h_k^l (n Fr: the second MSM's scalars) | 1 / h_k (n Fr) | -J_j (l Fr: the scalars of the MSM over
// [tau^j]_1) | g = sum gamma_k (1 Fr) | the partial rows. point_mode 0: h_k = d_points[k]; 1: h_k = d_points[0]^k. Value (k, t) is the Fr at
// d_values + 32 (k item_stride + t t_stride) bytes. omega_l_inv, inv_l: host pointers, read before the call returns.
struct VcWork { void *s, *hinv, *neg_j, *g, *part_g, *part_j; };
size_t verify_cosets_work_bytes(size_t n, uint32_t log2l);
VcWork verify_cosets_layout(size_t n, uint32_t log2l, void* d_work);
keaki_status verify_cosets_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const void* d_values, size_t item_stride,
                                       size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, const VcWork& w);
// kzg verify_sets (kzg_sets.hip), n items of k points each, 1 <= n, 1 <= k <= KEAKI_VERIFY_SETS_K_MAX <= item_stride, n * k < 2^31. The workspace of a call
// (verify_sets_work_bytes) holds the k + 1 scalar rows of the batched MSM over the proofs (row t at s + 32 (t n + i): -gamma_i Z_(i,0) | gamma_i Z_(i,t) | gamma_i) |
// the weights 1 / Z_i'(z_(i,j)) (n k Fr) | -J_t (the scalars of the MSM over [tau^t]_1) | g = sum gamma_i | the partial rows | (point_mode 1) the derived points.
// point_mode 0: z_(i,j) = the Fr at d_points + 32 (i item_stride + j); 1: omega^idx, idx the u32 at d_points + 4 (i item_stride + j), omega a HOST pointer read
// before the call returns. Value (i, j) is the Fr at d_values + 32 (i item_stride + j). verify_sets_pairs_run: d_sums_aff = L (d_l_jac), R_1 .. R_k (d_rows_jac[1 ..
// k]) affine, (0, 0) for the identity; d_ps_aff = the same with -L in front (the first slots of the k + 1 pairings).
struct VsWork { void *s, *w, *neg_j, *g, *part, *pts; };
size_t verify_sets_work_bytes(size_t n, size_t k, int point_mode);
VsWork verify_sets_layout(size_t n, size_t k, void* d_work);
keaki_status verify_sets_scalars_run(keaki_hip_ctx* ctx, const void* d_gammas, const void* d_points, int point_mode, const uint64_t* omega, const void* d_values,
                                     size_t item_stride, size_t k, size_t n, const VsWork& w);
keaki_status verify_sets_pairs_run(keaki_hip_ctx* ctx, const void* d_l_jac, const void* d_rows_jac, size_t k, void* d_sums_aff, void* d_ps_aff);
// kzg set_pairs / verify_sets_each. Fr side (kzg_sets.hip, the rows instantiations of k_vs_polys): for the m items [first, first + m) of the caller's arrays
// (m * kp < 2^31, kp = the power of two >= k) d_rows_i[(i << log2 kp) + t] = -I_(first + i, t) (t < k, zeros up to kp; canonical integers, or with `mont` the
// Montgomery form the batched MSM takes) and d_rows_z[i k + t] = Z_(first + i, t) (t < k, canonical; Z is monic, the coefficient of X^k is not stored).
// d_w: m k Fr (the weights), d_pts: m k Fr (point_mode 1 only); d_rows_i doubles as the weights' scratch. G2 side (kzg_set_pairs.hip): the window table over the
// first n_bases G2 points (set_rows_plan.h: sr_table_bytes) | d_xyzz[i] = [tau^k]_2 + sum_t rows_z[i][t] [tau^t]_2 by the table walk in S slices per item |
// m XYZZ points -> affine, (0,0) for the identity. Verdict side: kzg_set_each_pair.hip (the fused kernel) and the pieces of route 2 (set_each_*; gt_product.hip).
keaki_status set_pairs_rows_run(keaki_hip_ctx* ctx, const void* d_points, int point_mode, const uint64_t* omega, const void* d_values, size_t item_stride, size_t k,
                                size_t first, size_t m, bool mont, void* d_w, void* d_pts, void* d_rows_i, void* d_rows_z);
keaki_status g2_fb_tables_run(keaki_hip_ctx* ctx, const void* d_bases, uint32_t n_bases, void* d_table, uint32_t wb);   // table[(b windows + j) entries + d] = d 2^(wb j) bases[b]
keaki_status set_rows_g2_run(keaki_hip_ctx* ctx, const void* d_table, uint32_t wb, const void* d_rows_z, size_t k, uint32_t S, const void* d_tau_k_g2, size_t m,
                             void* d_xyzz);
keaki_status set_rows_affine_g2_run(keaki_hip_ctx* ctx, const void* d_xyzz, size_t m, void* d_out_aff);
// d_status[i] = 0 iff e(a_i, g2) == e(proof_i, z2_i); R = (proof_i or z2_i is the identity): with a_i or R an identity the item is valid iff both are. ONE launch
// of n <= ws_items <= pairing_launch_items() items over the final exponentiation's slots at d_ws; d_lines_g2: g2's line table.
keaki_status pairing2v_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_proofs, const void* d_z2, size_t n, const void* d_lines_g2, void* d_ws,
                           size_t ws_items, void* d_status);
// route 2: d_ps = [a_i : m | -proof_i : m], d_qs = [g2 : m | z2_i : m] (the 2m pairs of miller_only_run) | d_out[i] = d_a[i] d_b[i] (12 Fq each, the 2^256 form of
// miller_only_run) | the status bytes from the 384 serialised bytes per item and the identity rule
keaki_status set_each_points_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_proofs, const void* d_z2, size_t m, void* d_ps, void* d_qs);
keaki_status gt_pair_product_run(keaki_hip_ctx* ctx, const void* d_a, const void* d_b, size_t m, void* d_out);
keaki_status set_each_status_run(keaki_hip_ctx* ctx, const void* d_gt_bytes, const void* d_a, const void* d_proofs, const void* d_z2, size_t m, void* d_status);
// GT product (gt_product.hip): d_out = prod of the n Fq12 at d_in (12 Fq each, 2^256 Montgomery form, slot 2k + parity: what miller_only_run writes and
// final_exp_only_run reads), n < 2^31; n = 0: one. d_part: gt_product_part_bytes() of workspace (may not overlap d_in or d_out).
size_t gt_product_part_bytes();
keaki_status gt_product_run(keaki_hip_ctx* ctx, const void* d_in, size_t n, void* d_part, void* d_out);
// kzg coset_pairs. Fr side (kzg_cosets.hip, the PAIRS / ROWS instantiations of the kernels above): d_c_out[k] = h_k^l (Montgomery), d_hinv[k] = 1 / h_k for the n
// items of a call | d_rows[(i << log2l) + j] = -a_(first + i, j) for the m items of a launch chunk (m * l < 2^31), canonical integers or (mont) Montgomery form.
// Group side (kzg_coset_pairs.hip): the window table of the first l SRS points (coset_rows_plan.h: cr_table_bytes) | d_xyzz[i] = C_(first + i) + sum_j
// rows[i][j] [tau^j]_1 by the table walk in S slices per item, or from the Jacobian sums of msm_g1_batch_run | m XYZZ points -> affine, (0,0) for the identity.
keaki_status coset_pairs_shifts_run(keaki_hip_ctx* ctx, const void* d_points, int point_mode, uint32_t log2l, size_t n, void* d_c_out, void* d_hinv);
keaki_status coset_pairs_rows_run(keaki_hip_ctx* ctx, const void* d_values, size_t item_stride, size_t t_stride, const void* d_hinv, uint32_t log2l,
                                  const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t first, size_t m, bool mont, void* d_rows);
keaki_status coset_table_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2l, uint32_t wb, void* d_table);
keaki_status coset_rows_table_run(keaki_hip_ctx* ctx, const void* d_table, uint32_t wb, const void* d_rows, uint32_t log2l, uint32_t S, const void* d_coms,
                                  int com_stride, size_t first, size_t m, void* d_xyzz);
keaki_status coset_rows_join_run(keaki_hip_ctx* ctx, const void* d_sums_jac, const void* d_coms, int com_stride, size_t first, size_t m, void* d_xyzz);
keaki_status coset_rows_affine_run(keaki_hip_ctx* ctx, const void* d_xyzz, size_t m, void* d_out_aff);
// layout moves around the final sum (no arithmetic): n <= 64 affine points -> normalised Jacobian | the normalised Jacobian sums L, R -> d_out_lr_aff[0], [1] affine
keaki_status verify_batch_aff_to_jac_run(keaki_hip_ctx* ctx, const void* d_in_aff, uint32_t n, void* d_out_jac);
keaki_status verify_batch_jac_to_aff_run(keaki_hip_ctx* ctx, const void* d_l_jac, const void* d_r_jac, void* d_out_lr_aff);
// kzg verify_each (kzg_each.hip, kzg_each_pair.hip). Items [first, first + n) of the caller's arrays (first + n < 2^31):
// d_lhs_out[i] = C_((first + i) * com_stride) - y g1 + z proof and d_neg_proof_out[i] = -proof, affine, i < n; point_mode 1: z = d_points[0]^(first + i);
// d_tab_g1: the wb-bit window table of g1
keaki_status verify_each_g1_run(keaki_hip_ctx* ctx, const void* d_coms, int com_stride, const void* d_tab_g1, uint32_t wb, const void* d_points, int point_mode,
                                const void* d_values, const void* d_proofs, size_t first, size_t n, void* d_lhs_out, void* d_neg_proof_out);
// d_status[i] = 0 iff e(p1_i, A) e(p2_i, B) == 1, A and B given by their line tables; ONE launch of n <= ws_items <= pairing_launch_items() items over
// the final exponentiation's slots at d_ws (pairing_slot_bytes() per item of ws_items). An identity in either slot: 0 iff both are.
keaki_status pairing2_fixed_run(keaki_hip_ctx* ctx, const void* d_p1, const void* d_p2, size_t n, const void* d_lines_a, const void* d_lines_b, void* d_ws,
                                size_t ws_items, void* d_status);
size_t pairing_slot_bytes();
keaki_status verify_each_tau_inf_run(keaki_hip_ctx* ctx, const void* d_lhs, size_t n, void* d_status);   // [tau]_2 = identity: status = (lhs is not the identity)
keaki_status verify_each_count_run(keaki_hip_ctx* ctx, const void* d_status, size_t n, void* d_bad2);    // d_bad2: u64 count, u64 first index, added to
// compressed point wire format (point_codec.hip): one lane per point; n < 2^31. d_bad2: u64 count, u64 first index (over base + i: the host forms run in
// chunks), added to by every launch; d_status (optional): one byte per item
keaki_status point_compress_run(keaki_hip_ctx* ctx, bool g2, const void* d_pts, size_t n, void* d_out);
keaki_status point_decompress_run(keaki_hip_ctx* ctx, bool g2, const void* d_bytes, size_t n, uint64_t base, void* d_out, void* d_status, void* d_bad2);
// psi(Q) == [6 z^2]Q per point; an outsider gets status 3 (d_status given) and, with `clear`, all-zero words in place
keaki_status g2_subgroup_run(keaki_hip_ctx* ctx, void* d_pts, size_t n, uint64_t base, void* d_status, bool clear, void* d_bad2);
// batched small MSM and batched quotient (msm_batch.hip). Rows of n <= N_BATCH_MAX scalars run the batch kernels, msm_batch_rows_per_pass rows
// at a time (workspace: 32 B per scalar of a pass, at most MSM_BATCH_CANON_BYTES unless one row is longer, + 128 B per row and window); longer rows, and
// calls whose workspace is refused with KEAKI_ERR_OOM, run msm_g1_run row by row. d_out_jac: m x 96 B. Asynchronous on ctx->stream.
constexpr size_t N_BATCH_MAX = 16384, MSM_BATCH_CANON_BYTES = (size_t)1 << 28, MSM_BATCH_ROWS_MAX = 16384;
int msm_batch_window(size_t n);                          // window bits c of the batch plan msm_make_plan(n, c): 4 .. 9
size_t msm_batch_rows_per_pass(size_t n, size_t m);      // n >= 1
keaki_status msm_g1_batch_run(keaki_hip_ctx* ctx, const void* d_points, size_t srs_len, const void* d_table, int c_table, const void* d_scalars, size_t n,
                              size_t m, size_t stride, void* d_out_jac);
// row j < m: d_q[j * qstride + i - 1] = Q_i (1 <= i < n), d_values[j] = Q_0 (d_values may be null) for Q_i = c_i + z_j Q_(i+1) over row j of d_coeffs
keaki_status fr_quotient_batch_run(keaki_hip_ctx* ctx, const void* d_coeffs, size_t n, size_t m, size_t stride, const void* d_points, void* d_q, size_t qstride,
                                   void* d_values);
// batched FK23 (fk_batch.hip): domains of 2 .. 2^FKB_LOG2D_MAX run the batch kernels in passes of whole rows, fkb_rows_per_pass at a time (a
// multiple of 64 unless m is smaller; FKB_ROW_BYTES << log2d bytes of workspace per row, at most FKB_PASS_BYTES a pass). The caller (api.hip)
// reserves for `cap` rows, halving on KEAKI_ERR_OOM, runs fkb_tables_run once (-> omega_2d^k, the table fk_cache_ensure takes) and every pass
// with the same cap; larger domains, d = 1 and refused workspaces run the single pipeline row by row. Asynchronous on ctx->stream.
constexpr uint32_t FKB_LOG2D_MAX = 12;
constexpr size_t FKB_PASS_BYTES = (size_t)1 << 28, FKB_ROW_BYTES = 288, FKB_ROWS_MAX = 16384;
size_t fkb_rows_per_pass(uint32_t log2d, size_t m);
keaki_status fkb_reserve(keaki_hip_ctx* ctx, uint32_t log2d, size_t rows);
const void* fkb_tables_run(keaki_hip_ctx* ctx, uint32_t log2d, size_t rows, const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* omega_d_inv_or_null);
keaki_status fkb_pass_run(keaki_hip_ctx* ctx, const void* d_hat_s, uint32_t log2d, size_t cap, const void* d_rows, size_t n, uint32_t rows, size_t stride,
                          const uint64_t* inv_d_or_null, const uint64_t* inv_2d, void* d_proofs, const void** d_coeffs_out);
// the stage machinery of FK23 for other callers (fft_g1.hip): an in-place size-2^log2n transform, decimation in frequency (d_tw: root^k, k < n / 2;
// position q out holds X[brev(q)]) | the window-table workspace of the per-lane-scalar ladders (null: private memory) and the lanes one launch may cover
keaki_status g1_dif_run(keaki_hip_ctx* ctx, void* d_pts_jac, uint32_t log2n, const void* d_tw);
void* ladder_workspace(keaki_hip_ctx* ctx, uint32_t lanes, uint32_t* lanes_per_launch);
// vec_update (vec_update.hip). The tables of (srs, d = 2^log2d): a (d affine) | u (d affine) | omega_d^-i (d Fr) | 1 / (omega_d^t - 1) (d Fr). upd_apply_run: k >= 1
// entries (d_idx: u32, d_deltas: Fr) onto d_com (normalised Jacobian, or null) and d_proofs (d affine, or null); an index >= d does nothing. Asynchronous on ctx->stream.
size_t upd_table_bytes(uint32_t log2d);
keaki_status upd_tables_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2d, const uint64_t* omega_d_inv, const uint64_t* inv_d, void* d_tab);
keaki_status upd_apply_run(keaki_hip_ctx* ctx, const void* d_tab, uint32_t log2d, const uint64_t* inv_d, const void* d_idx, const void* d_deltas, size_t k,
                           void* d_com, void* d_proofs);
// KZG set openings (kzg_multi.hip). set_polys_run: Z (k + 1 Fr; d_zc may be null when d_ic is), the weights 1 / Z'(z_j) (k Fr) and, with values, the
// interpolant (k Fr) of 1 <= k <= KEAKI_SET_MAX DISTINCT points, one workgroup. multi_quotient_run: d_q = the n - 1 coefficients of
// sum_j weight_j (p - p(z_j)) / (x - z_j) = (p - I) / Z and d_values[j] = p(z_j), for n >= 1 coefficients, in passes of 8 points. All on ctx->stream.
keaki_status set_polys_run(keaki_hip_ctx* ctx, const void* d_points, const void* d_values, size_t k, void* d_zc, void* d_weights, void* d_ic);
size_t multi_quotient_work_bytes(size_t n);
keaki_status multi_quotient_run(keaki_hip_ctx* ctx, const void* d_c, size_t n, const void* d_points, const void* d_weights, size_t k, void* d_q, void* d_values,
                                void* d_work);
// verify_multi: d_out_a_aff = C - I1, d_out_z_aff = Z2 (affine) from the commitment and the two MSM results (normalised or not)
keaki_status set_pair_points_run(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_i1_jac, const void* d_z2_jac, void* d_out_a_aff, void* d_out_z_aff);
// FK23 coset openings (fk_coset.hip; the split of a position's terms: fk_coset_plan.h). r = 2^(log2d - log2l) >= 2 everywhere. The scalar workspace
// (fkc_fr_bytes) holds tw = omega_2r^k, twi = omega_2r^-k (k < r), twr = omega_r^k (k < r / 2) and hat_a (l rows of 2r Fr, natural order, divided by 2r).
struct FkcPlan;
struct FkcScalars { void *tw, *twi, *twr, *hat_a; };
size_t fkc_fr_bytes(uint32_t log2d, uint32_t log2l);
size_t fkc_g_bytes(uint32_t log2d, uint32_t log2l, const FkcPlan& plan);
FkcScalars fkc_layout(uint32_t log2d, uint32_t log2l, void* d_fr_work);
keaki_status fkc_reserve_tab(keaki_hip_ctx* ctx, size_t lanes, uint32_t G, uint32_t* lanes_per_launch);
keaki_status fkc_tables_run(keaki_hip_ctx* ctx, uint32_t log2r, const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const FkcScalars& s);
keaki_status fkc_hat_s_run(keaki_hip_ctx* ctx, const void* d_srs, uint32_t log2d, uint32_t log2l, const void* d_tw, void* d_hat_s);
keaki_status fkc_scalars_run(keaki_hip_ctx* ctx, uint32_t log2d, uint32_t log2l, const void* d_p, const uint64_t* inv_2r, const FkcScalars& s);
keaki_status fkc_open_run(keaki_hip_ctx* ctx, const void* d_hat_s, uint32_t log2d, uint32_t log2l, const FkcScalars& s, const FkcPlan& plan,
                          uint32_t lanes_per_launch, void* d_g_work, void* d_proofs_aff);
keaki_status selftest_u29_run(keaki_hip_ctx* ctx, uint32_t blocks, uint32_t iters, uint32_t seed, void* d_mismatches);
keaki_status selftest_field_run(keaki_hip_ctx* ctx, uint32_t blocks, uint32_t iters, uint32_t seed, void* d_mismatches);
// field probe (field_probe.hip): op `op` of keaki_field_op on n records at d_operands (field_probe_padded(op, n) records: lane-pair ops run whole
// waves), raw results to d_out (n records). Checks op and n itself (KEAKI_ERR_BAD_ARG, nothing launched).
bool field_probe_is_pair(uint32_t op);
size_t field_probe_padded(uint32_t op, size_t n);
keaki_status field_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out);
// tower probe (tower_probe.hip, tower_probe_wide.hip): op `op` of keaki_tower_op on n records at d_operands (tower_probe_padded(op, n) records: whole
// waves of 32 lane pairs or of 4 rows), twelve Fq per record to d_out (n records). Checks op and n itself (KEAKI_ERR_BAD_ARG, nothing launched).
bool tower_probe_is_wide(uint32_t op);
size_t tower_probe_padded(uint32_t op, size_t n);
keaki_status tower_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out);
// point probe (point_probe.hip, point_probe_g2.hip): op `op` of keaki_point_op on n records at d_operands; whole waves run, so d_operands AND d_out
// hold point_probe_padded(n) records (d_out zeroed by the caller) and d_table point_probe_table_bytes(op, n) bytes (0: none needed). Checks op and
// n itself (KEAKI_ERR_BAD_ARG, nothing launched).
size_t point_probe_padded(size_t n);
size_t point_probe_table_bytes(uint32_t op, size_t n);
keaki_status point_probe_run(keaki_hip_ctx* ctx, uint32_t op, const void* d_operands, size_t n, void* d_out, void* d_table);

}  // namespace keaki_internal
