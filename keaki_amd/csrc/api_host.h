// The host layer's private interface (not installed): what more than one host translation unit of the C ABI needs -- api.hip, which defines
// everything that is only declared here, and the family files beside it (api_kzg.hip). Host code only: no kernel and no launch site.
#pragma once
#include "internal.h"

#include <algorithm>
#include <set>

// An SRS handle is device memory, not context state: every context ON THE SAME DEVICE may pass it to msm / open / open_fk (read-only use
// of the points, the window tables and the cached FK23 transform), so N host threads with a context each share ONE set of tables.
// `mu` guards the lazily built members (table, fk); `acct` is the context whose keaki_hip_ctx_memory counts them.
struct SrsHandle {
  const void* d = nullptr;
  size_t n = 0;
  bool owned = false;
  int device = -1;
  std::recursive_mutex mu;
  keaki_hip_ctx* acct = nullptr;
  // precomputed window tables (keaki_hip_srs_g*_precompute): table[w * n + i] = 2^(offset_w) * P_i
  void* table = nullptr;
  size_t table_bytes = 0;
  int c_table = 0;
};
// A device table derived from the points of a G1 handle for the LAST requested shape, reused by later calls on the handle. Owned by
// srs_cache_ensure: the key names a table only when its build was enqueued in full (an unused part stays -1), bytes is what p holds (and `acct` counts).
struct SrsCache {
  void* p = nullptr;
  int key[2] = {-1, -1};
  size_t bytes = 0;
  bool holds(int k0, int k1 = -1) const { return key[0] == k0 && key[1] == k1; }
};
// fk: FK23, hat_s = DFT_2d(reversed SRS), 2d Jacobian points, key log2d | upd: vec_update, the update tables of d (vec_update.hip: a | u | omega_d^-i |
// 1 / (omega_d^t - 1)), key log2d | fkc: FK23 coset openings, the l transforms hat_s_j = DFT_2r(row j of the SRS, reversed), 2d Jacobian points
// (fk_coset.hip), key (log2d, log2l) | cr: kzg coset_pairs, the window table over the first l points (kzg_coset_pairs.hip, coset_rows_plan.h), key (log2l, wb).
// The four are independent of each other; a new cache is added HERE (srs_free walks them). The G2 handle has one: sr, kzg set_pairs, the window table over
// the first kb points (kzg_set_pairs.hip, set_rows_plan.h), key (kb, wb); base-major, so it serves every k <= kb.
struct keaki_hip_srs_g1 : SrsHandle {
  SrsCache fk, upd, fkc, cr;
  template <class F> void for_each_cache(F&& f) { for (SrsCache* c : {&fk, &upd, &fkc, &cr}) f(*c); }
};
struct keaki_hip_srs_g2 : SrsHandle {
  SrsCache sr;
  template <class F> void for_each_cache(F&& f) { f(sr); }
};

namespace keaki_internal {

// roctx ranges around the kernel families, visible to `rocprofv3 --marker-trace`; no-ops without the marker library (api.hip: Roctx)
struct RoctxScope {
  bool on;
  explicit RoctxScope(const char* name);
  ~RoctxScope();
};
#define TRACE_SCOPE(name) RoctxScope roctx_scope_(name)
// The contexts that are alive: an SRS handle is shared by every context of its device, and whoever frees it (or rebuilds its FK23 transform)
// must be able to undo the byte accounting on the context that built the tables -- if that context still exists.
extern std::mutex g_live_mu;
extern std::set<keaki_hip_ctx*> g_live_ctx;
// runs `f(acct)` when acct is a live context. Under g_live_mu ONLY: the caller may already hold its own context's lock, and taking another
// context's lock from here would order the two locks both ways (thread A: ctx1 -> live -> ctx2, thread B: ctx2 -> live). What f touches --
// the byte count `mem_tables` -- is an atomic for that reason.
template <class Fn>
void with_live_ctx(keaki_hip_ctx* acct, Fn f) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  if (acct && g_live_ctx.count(acct)) f(acct);
}
// saturating subtraction on the byte count (a handle freed twice over, or booked before a trim, must not wrap it)
inline void mem_sub(std::atomic<size_t>& m, size_t v) {
  size_t cur = m.load();
  while (!m.compare_exchange_weak(cur, cur - std::min(cur, v))) {}
}
constexpr size_t G1_AFF_BYTES = 64, G2_AFF_BYTES = 128, G1_JAC_BYTES = 96, G2_JAC_BYTES = 192;

#define CTX_GUARD(ctx)                                \
  if (!(ctx)) return KEAKI_ERR_BAD_ARG;               \
  std::lock_guard<std::recursive_mutex> lock_((ctx)->mu);       \
  keaki_internal::DeviceScope dev_((ctx)->device);              \
  if (!dev_.ok) return fail(ctx, KEAKI_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)

keaki_status download(keaki_hip_ctx* ctx, void* host, const void* dev, size_t bytes);
// How the caller's HOST arrays reach the device, for every host-array entry: the copies go on the context's stream, or after begin(true) on
// the copy stream, where `put` makes the stream that reads a piece wait for it. The feed also keeps the rule of the header: a call that
// FAILS returns, too, only when no copy reads the caller's arrays any more and nothing of it is left on a side stream -- unless the call
// said `settled()` (where its own download has synchronised), the destructor drains every stream that carried a copy or was handed in.
struct CopyFeed {
  keaki_hip_ctx* ctx;
  bool side = false;
  hipStream_t drain[3] = {nullptr, nullptr, nullptr};
  int n_drain = 0;
  explicit CopyFeed(keaki_hip_ctx* c) : ctx(c) {}
  ~CopyFeed() { for (int i = 0; i < n_drain; i++) (void)hipStreamSynchronize(drain[i]); }
  CopyFeed(const CopyFeed&) = delete;
  CopyFeed& operator=(const CopyFeed&) = delete;
  void also_drain(hipStream_t s) { if (std::find(drain, drain + n_drain, s) == drain + n_drain) drain[n_drain++] = s; }
  void settled() { n_drain = 0; }
  keaki_status closed_by(keaki_status last) { if (last == KEAKI_OK) settled(); return last; }      // `last`: of the call's last step, which synchronises
  keaki_status begin(bool side_stream) {
    if (!side_stream) return KEAKI_OK;
    ST_TRY(ctx->pipe.ready(ctx));
    // the copy stream starts behind whatever the context's stream holds (an earlier call's kernels may still read the destination)
    HIP_TRY(ctx, hipEventRecord(ctx->pipe.done[0], ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipe.copy_stream, ctx->pipe.done[0], 0));
    side = true;
    return KEAKI_OK;
  }
  // piece j of the call, host to device; `waiter` (default: the context's stream) is the stream whose kernels read it
  keaki_status put(size_t j, void* dst, const void* src, size_t bytes, hipStream_t waiter = nullptr) {
    const hipStream_t cs = side ? ctx->pipe.copy_stream : ctx->stream;
    also_drain(cs);
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
    if (!side) return KEAKI_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->pipe.in[j & 1], cs));
    HIP_TRY(ctx, hipStreamWaitEvent(waiter ? waiter : ctx->stream, ctx->pipe.in[j & 1], 0));
    return KEAKI_OK;
  }
};
keaki_status upload(CopyFeed& feed, DevBuf& b, const void* host, size_t bytes);
keaki_status download(CopyFeed& feed, void* host, const void* dev, size_t bytes);     // the last step of a successful call
// The items of a KZG host form on their way to the device, told ONCE what the call has: ONE commitment (com_stride 0) goes to `com_slot`, omega alone
// (point_mode 1) to `omega_slot`, or where the call keeps no such slot (null) to the front of the per-item buffer; n commitments go to io_e, n points to io_c, the n
// proofs (null: none) to io_b. reserve() covers every buffer before the first copy is enqueued: a reserve that grows a buffer waits for ctx->stream only. put(feed,
// what) enqueues the inputs `what` selects, in the order commitment, points, proofs; put(feed, dst, src, bytes) one of the call's own arrays; d_*(): where each is read.
struct ItemStager {
  enum : unsigned { ONE_COM = 1, COMS = 2, OMEGA = 4, POINTS = 8, PROOFS = 16, COM = ONE_COM | COMS, PTS = OMEGA | POINTS, ALL = COM | PTS | PROOFS };
  keaki_hip_ctx* ctx;
  const void* com; int32_t com_stride; void* com_slot;
  const void* points; int32_t point_mode; void* omega_slot;
  const void* proofs; size_t n, piece = 0;
  void* d_com() const { return !com_stride && com_slot ? com_slot : ctx->io_e.p; }
  void* d_points() const { return point_mode && omega_slot ? omega_slot : ctx->io_c.p; }
  void* d_proofs() const { return ctx->io_b.p; }
  keaki_status reserve() {
    if (proofs) ST_TRY(keaki_internal::reserve(ctx, ctx->io_b, n * G1_AFF_BYTES));
    if (d_points() == ctx->io_c.p) ST_TRY(keaki_internal::reserve(ctx, ctx->io_c, (point_mode ? 1 : n) * 32));
    return d_com() == ctx->io_e.p ? keaki_internal::reserve(ctx, ctx->io_e, (com_stride ? n : 1) * G1_AFF_BYTES) : KEAKI_OK;
  }
  keaki_status put(CopyFeed& feed, void* dst, const void* src, size_t bytes) { return feed.put(feed.side ? piece++ : 0, dst, src, bytes); }
  keaki_status put(CopyFeed& feed, unsigned what) {
    if (what & (com_stride ? COMS : ONE_COM)) ST_TRY(put(feed, d_com(), com, (com_stride ? n : 1) * G1_AFF_BYTES));
    if (what & (point_mode ? OMEGA : POINTS)) ST_TRY(put(feed, d_points(), points, (point_mode ? 1 : n) * 32));
    return proofs && (what & PROOFS) ? put(feed, d_proofs(), proofs, n * G1_AFF_BYTES) : KEAKI_OK;
  }
};
// The two pairings of a verdict in ONE launch; `sums_out_aff` (or null) takes the 128 bytes of d_ps, enqueued before the download of the 768 GT bytes, which synchronises.
keaki_status pair2_verdict(keaki_hip_ctx* ctx, const void* d_ps, const void* d_qs, void* d_gt, uint64_t* sums_out_aff, int32_t* ok_out);
// first-touches the caller's OUTPUT buffer from the host while the kernels that produce the data run (api.hip has the measurements)
void prefault_out(const keaki_hip_ctx* ctx, void* p, size_t bytes);

// The device pair {count of bad items, first bad index} of a call with a verdict per item, in a 16-byte slot: begin() writes {0, ~0} on ctx->stream, the
// call's kernels add to the slot, end() downloads it (which synchronises) and hands the two numbers to the caller.
struct BadTally {
  keaki_hip_ctx* ctx;
  void* slot;
  keaki_status begin() {
    const uint64_t init[2] = {0, ~0ull};
    HIP_TRY(ctx, hipMemcpyAsync(slot, init, 16, hipMemcpyHostToDevice, ctx->stream));
    return KEAKI_OK;
  }
  keaki_status end(uint64_t* n_bad, uint64_t* first_bad) {
    uint64_t res[2];
    ST_TRY(download(ctx, res, slot, 16));
    *n_bad = res[0];
    if (first_bad) *first_bad = res[1];
    return KEAKI_OK;
  }
};

// (table, window target) of a handle, read under its lock: another context may be building the tables right now
template <class H>
std::pair<const void*, int> srs_tables(const H* srs) {
  std::lock_guard<std::recursive_mutex> hl(const_cast<H*>(srs)->mu);
  return {srs->table, srs->c_table};
}
// a handle may be used by any context of the device it lives on
#define SRS_CHECK(ctx, srs, what)                                                                                                     \
  if ((srs)->device != (ctx)->device)                                                                                                 \
    return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: the SRS handle lives on device %d, this context on device %d", what, (srs)->device, (ctx)->device)
// ... and must hold the k points the call reads: `too_short` is the family's message when it does not
keaki_status srs_holds(keaki_hip_ctx* ctx, const SrsHandle* srs, const char* what, size_t k, const char* too_short);
// The ONE owner of every cache of a handle: afterwards c.p is the table of key (k0, k1), `bytes` long, that `build(c.p)` enqueues on the
// context's stream; the caller holds srs->mu. A table of another key is dropped first (after the stream's work that may read it), the new
// one is allocated through dev_alloc and named only once its build is enqueued in full; on every exit -- a refused allocation
// included -- c.bytes and the `tables` count of the handle's accounting context (srs->acct, as for the window tables) say what c.p holds.
template <class H, class Build>
keaki_status srs_cache_ensure(keaki_hip_ctx* ctx, H* srs, SrsCache& c, int k0, int k1, size_t bytes, Build build) {
  if (c.holds(k0, k1)) return KEAKI_OK;
  auto book = [&](size_t now) {
    const size_t before = c.bytes;
    with_live_ctx(srs->acct, [&](keaki_hip_ctx* a) { mem_sub(a->mem_tables, before); a->mem_tables += now; });
    c.bytes = now;
  };
  c.key[0] = c.key[1] = -1;
  if (c.p) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(c.p); c.p = nullptr; book(0); }
  ST_TRY(dev_alloc(ctx, &c.p, bytes));
  book(bytes);
  ST_TRY(build(c.p));
  c.key[0] = k0; c.key[1] = k1;
  return KEAKI_OK;
}

// chunk unit of the host-array batches (api.hip: pipelined): two rounds of the GT exponentiation kernel
constexpr size_t PIPE_CHUNK = 65536;
// window widths of the fixed-base tables: 16 bits for bases that outlive a batch (generators: per context, [tau]_2: per setup), 13 bits for the
// commitment's table (rebuilt per batch in the per-item-pairing path), 8 bits for the small tables of small batches (api.hip: FB_TABLES_MIN)
constexpr uint32_t FB_WB_LONG = 16, FB_WB_BATCH = 13, FB_WB_SMALL = 8;
// g2 in tmp_c for the pairing's second slot (src/kem.rs:30), and once per context the generators' 16-bit tables and g2's line sequence (G2Prepared)
keaki_status generator_tables(keaki_hip_ctx* ctx, bool use_tables);
// the small tables of g2 (from the generator at d_g2_generator) and room for [tau]_2's: encapsulate below FB_TABLES_MIN items and kzg verify
keaki_status small_g2_tables(keaki_hip_ctx* ctx, const void* d_g2_generator);
// the small table of g1: kzg verify, and the fused route of encap_multi while the context has no long tables
keaki_status small_g1_table(keaki_hip_ctx* ctx);
// the two constants of the batch read back to the host: one synchronisation, for callers whose host copies did not come along. d_com null: [tau]_2 only
keaki_status read_constants(keaki_hip_ctx* ctx, const void* d_tau, const void* d_com, uint64_t* tau_host, uint64_t* com_host);

}  // namespace keaki_internal
