// libkeaki_hip.so -- C ABI (include/keaki_hip.h) over the gfx950 kernels. Host side only does
// launch plumbing: workspace management, stream ordering, error codes. No arithmetic happens on
// the CPU here and there is no CPU fallback: without a gfx950 device every entry point fails.
#include "api_host.h"
#include "host_plan.h"
#include "encap_multi_plan.h"
#include "fk_coset_plan.h"
#include "coset_rows_plan.h"
#include "set_rows_plan.h"

#include <dlfcn.h>
#include <sys/mman.h>
#include <cctype>
#include <chrono>
#include <memory>
#include <thread>
#include <type_traits>
#include <vector>

using namespace keaki_internal;

namespace {
// roctx ranges around the kernel families (tracing), visible to `rocprofv3 --marker-trace`. The marker library is
// looked up at run time so that the ABI has no link-time dependency on the profiler; without it the scopes are no-ops.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_LAZY | RTLD_LOCAL);
    if (h) {
      push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!push || !pop) push = nullptr;
    }
  }
};
const Roctx& roctx() { static Roctx r; return r; }
thread_local std::string g_create_error;
}  // namespace

namespace keaki_internal {

RoctxScope::RoctxScope(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
RoctxScope::~RoctxScope() { if (on) roctx().pop(); }
std::mutex g_live_mu;
std::set<keaki_hip_ctx*> g_live_ctx;

keaki_status fail(keaki_hip_ctx* ctx, keaki_status code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf; else g_create_error = buf;
  return code;
}

keaki_status dev_alloc(keaki_hip_ctx* ctx, void** p, size_t bytes) {
  if (ctx && ctx->tune.alloc_limit && bytes > ctx->tune.alloc_limit)
    return fail(ctx, KEAKI_ERR_OOM, "allocation of %zu bytes refused by keaki_hip_debug_set_alloc_limit(%zu)", bytes, ctx->tune.alloc_limit);
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? KEAKI_ERR_OOM : KEAKI_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  }
  if (ctx && ctx->poison_new >= 0 && bytes) {          // keaki_hip_debug_poison_workspaces: complete before any stream of the call can touch the memory
    hipError_t f = hipMemsetAsync(*p, ctx->poison_new, bytes, ctx->stream);
    if (f == hipSuccess) f = hipStreamSynchronize(ctx->stream);
    if (f != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(*p); *p = nullptr;
      return fail(ctx, KEAKI_ERR_HIP, "poison fill of %zu bytes failed: %s", bytes, hipGetErrorString(f));
    }
  }
  return KEAKI_OK;
}

keaki_status reserve(keaki_hip_ctx* ctx, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return KEAKI_OK;
  if (b.p) {
    // the buffer may still be in use by enqueued work
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  ST_TRY(dev_alloc(ctx, &b.p, want));
  b.cap = want;
  return KEAKI_OK;
}

keaki_status launch_check(keaki_hip_ctx* ctx, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, KEAKI_ERR_HIP, "launch %s failed: %s", what, hipGetErrorString(e));
  return KEAKI_OK;
}

keaki_status download(keaki_hip_ctx* ctx, void* host, const void* dev, size_t bytes) {
  if (bytes) HIP_TRY(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return KEAKI_OK;
}
keaki_status upload(CopyFeed& feed, DevBuf& b, const void* host, size_t bytes) {
  ST_TRY(reserve(feed.ctx, b, bytes ? bytes : 16));
  return feed.put(0, b.p, host, bytes);
}
keaki_status download(CopyFeed& feed, void* host, const void* dev, size_t bytes) {     // the last step of a successful call
  return feed.closed_by(download(feed.ctx, host, dev, bytes));
}
keaki_status pair2_verdict(keaki_hip_ctx* ctx, const void* d_ps, const void* d_qs, void* d_gt, uint64_t* sums_out_aff, int32_t* ok_out) {
  ST_TRY(pairing_run(ctx, d_ps, d_qs, 1, 2, d_gt));
  uint8_t gt[768];
  if (sums_out_aff) HIP_TRY(ctx, hipMemcpyAsync(sums_out_aff, d_ps, 128, hipMemcpyDeviceToHost, ctx->stream));
  ST_TRY(download(ctx, gt, d_gt, 768));
  *ok_out = memcmp(gt, gt + 384, 384) == 0 ? 1 : 0;
  return KEAKI_OK;
}
keaki_status srs_holds(keaki_hip_ctx* ctx, const SrsHandle* srs, const char* what, size_t k, const char* too_short) {
  SRS_CHECK(ctx, srs, what);
  if (k > srs->n) return fail(ctx, KEAKI_ERR_TOO_LARGE, too_short, k, srs->n);
  return KEAKI_OK;
}

// The caller's OUTPUT buffer is usually fresh memory (calloc / vec![0; n] / numpy.zeros): its pages do not exist until first touched, and a
// device-to-host copy into such pages crawls (160 MB of ciphertexts: 30 ms instead of 3). Touch one byte per page from the host WHILE the
// kernels that produce the data are still running: the faults are taken off the critical path. The whole range is overwritten by the copy
// that follows. (Resident pages cost ~2 ns each.)
// Fresh pages are also asked to be transparent HUGE pages (madvise(MADV_HUGEPAGE) on the 2 MB-aligned interior: a hint, ignored where the
// kernel does not offer it): first touch of 160 MB takes 20.5 ms in 4 KB pages and 6.5 ms in 2 MB pages on the GPU boxes
// (bench_tools/ubench_thp_touch.py). At 2^20 items the faults hide behind the kernels either way (vec_encrypt 52.6 vs 52.0 ms); the hint matters
// where the output is large against the kernel time (GT bytes out: 384 B per item).
void prefault_out(const keaki_hip_ctx* ctx, void* p, size_t bytes) {
  if (!ctx->tune.host_prefault || !p || bytes < (1u << 20)) return;    // option host_prefault = 0: the library never writes to (or madvises) caller memory itself
  {
    // memory the HIP runtime knows (hipHostMalloc / hipHostRegister: resident by construction, and copies from and to it are truly asynchronous,
    // so a write from here could overtake an upload still reading the same array): nothing to touch
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess) {
      if (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeDevice) return;
    } else {
      (void)hipGetLastError();
    }
  }
  {
    const uintptr_t HP = (uintptr_t)2 << 20, a = ((uintptr_t)p + HP - 1) & ~(HP - 1), e = ((uintptr_t)p + bytes) & ~(HP - 1);
    if (e > a) (void)madvise((void*)a, e - a, MADV_HUGEPAGE);
  }
  volatile unsigned char* c = (volatile unsigned char*)p;
  for (size_t off = 0; off < bytes; off += 4096) c[off] = 0;
  c[bytes - 1] = 0;
}

keaki_status generator_tables(keaki_hip_ctx* ctx, bool use_tables) {
  KemState& k = ctx->kem;
  ST_TRY(reserve(ctx, ctx->tmp_c, G2_AFF_BYTES));
  ST_TRY(g2_generator_to(ctx, ctx->tmp_c.p));
  if (use_tables && !k.fb_ready) {
    const size_t FBL = fb_table_entries(FB_WB_LONG);
    ST_TRY(reserve(ctx, k.fb_g1_gen, FBL * G1_AFF_BYTES + G1_AFF_BYTES));
    ST_TRY(reserve(ctx, k.fb_g2_gen, FBL * G2_AFF_BYTES));
    ST_TRY(reserve(ctx, k.fb_com, fb_table_entries(FB_WB_BATCH) * G1_AFF_BYTES));
    ST_TRY(reserve(ctx, k.fb_tau.buf, FBL * G2_AFF_BYTES));
    void* g1pt = (char*)k.fb_g1_gen.p + FBL * G1_AFF_BYTES;   // scratch slot behind the table
    ST_TRY(g1_generator_to(ctx, g1pt));
    ST_TRY(g1_fb_table_run(ctx, g1pt, k.fb_g1_gen.p, FB_WB_LONG));
    ST_TRY(g2_fb_table_run(ctx, ctx->tmp_c.p, k.fb_g2_gen.p, FB_WB_LONG));
    k.fb_ready = true;
  }
  if (!k.g2gen_lines_ready) {
    ST_TRY(reserve(ctx, k.g2gen_lines, g2_prepared_bytes()));
    ST_TRY(g2_prepare_run(ctx, ctx->tmp_c.p, k.g2gen_lines.p));
    k.g2gen_lines_ready = true;
  }
  return KEAKI_OK;
}
keaki_status small_g2_tables(keaki_hip_ctx* ctx, const void* d_g2_generator) {
  KemState& k = ctx->kem;
  if (k.fbs_ready) return KEAKI_OK;
  const size_t FBX = fb_table_entries(FB_WB_SMALL);
  ST_TRY(reserve(ctx, k.fbs_g2_gen, FBX * G2_AFF_BYTES));
  ST_TRY(reserve(ctx, k.fbs_tau.buf, FBX * G2_AFF_BYTES));
  ST_TRY(g2_fb_table_run(ctx, d_g2_generator, k.fbs_g2_gen.p, FB_WB_SMALL));
  k.fbs_ready = true;                 // fbs_tau is not valid yet: it is only ever built behind this point
  return KEAKI_OK;
}
keaki_status small_g1_table(keaki_hip_ctx* ctx) {
  KemState& k = ctx->kem;
  if (k.fbs_g1_ready) return KEAKI_OK;
  const size_t FBX = fb_table_entries(FB_WB_SMALL);
  ST_TRY(reserve(ctx, k.fbs_g1_gen, FBX * G1_AFF_BYTES + G1_AFF_BYTES));
  void* g1pt = (char*)k.fbs_g1_gen.p + FBX * G1_AFF_BYTES;    // scratch slot behind the table
  ST_TRY(g1_generator_to(ctx, g1pt));
  ST_TRY(g1_fb_table_run(ctx, g1pt, k.fbs_g1_gen.p, FB_WB_SMALL));
  k.fbs_g1_ready = true;
  return KEAKI_OK;
}
keaki_status read_constants(keaki_hip_ctx* ctx, const void* d_tau, const void* d_com, uint64_t* tau_host, uint64_t* com_host) {
  HIP_TRY(ctx, hipMemcpyAsync(tau_host, d_tau, 128, hipMemcpyDeviceToHost, ctx->stream));
  if (d_com) HIP_TRY(ctx, hipMemcpyAsync(com_host, d_com, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return KEAKI_OK;
}

}  // namespace keaki_internal

namespace {

void resolve_timing(keaki_hip_ctx* ctx) {
  if (!ctx->timing_pending) return;
  if (hipEventSynchronize(ctx->ev[3]) == hipSuccess) {
    (void)hipEventElapsedTime(&ctx->last_bucket_ms, ctx->ev[1], ctx->ev[2]);
    (void)hipEventElapsedTime(&ctx->last_total_ms, ctx->ev[0], ctx->ev[3]);
  }
  ctx->timing_pending = false;
}
void resolve_fk_timing(keaki_hip_ctx* ctx) {
  if (!ctx->fk_timing_pending) return;
  if (hipEventSynchronize(ctx->fk_ev[3]) == hipSuccess) {
    (void)hipEventElapsedTime(&ctx->last_fk_ms[0], ctx->fk_ev[0], ctx->fk_ev[1]);
    (void)hipEventElapsedTime(&ctx->last_fk_ms[1], ctx->fk_ev[1], ctx->fk_ev[2]);
    (void)hipEventElapsedTime(&ctx->last_fk_ms[2], ctx->fk_ev[0], ctx->fk_ev[3]);
  }
  ctx->fk_timing_pending = false;
}

template <class H>
H* new_srs(keaki_hip_ctx* ctx, const void* d, size_t n, bool owned) {
  H* h = new H();
  h->d = d; h->n = n; h->owned = owned; h->device = ctx->device; h->acct = ctx;
  return h;
}
// `too_short` of srs_holds: the message of the MSM family and of the FK23 family
constexpr const char *SRS_SHORT_MSM = "msm: %zu scalars but the SRS holds %zu points", *SRS_SHORT_FK = "open_fk: %zu coefficients but the SRS holds %zu points";
// the FK23 transform of d = 2^log2d into srs->fk. d_tw: omega_2d^k, k < d, ready in stream order
keaki_status fk_cache_ensure(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_tw) {
  return srs_cache_ensure(ctx, srs, srs->fk, (int)log2d, -1, ((size_t)2 << log2d) * G1_JAC_BYTES,
                          [&](void* hat_s) { return fk_hat_s_run(ctx, srs->d, log2d, d_tw, hat_s); });
}
// How every FK23 entry starts: its pointers are there (`args_ok`) and log2d is in range, the handle lives on this device and holds the
// d = 2^log2d points (`too_short`: the family's message when it does not), and `hl` takes the handle's lock: the caches belong to the
// handle, one call per handle at a time.
keaki_status fk_enter(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, bool args_ok, const char* what, std::unique_lock<std::recursive_mutex>& hl,
                      const char* too_short = SRS_SHORT_FK) {
  if (!srs || !args_ok || log2d > 27) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: bad argument", what);
  ST_TRY(srs_holds(ctx, srs, what, (size_t)1 << log2d, too_short));
  hl = std::unique_lock<std::recursive_mutex>(srs->mu);
  return KEAKI_OK;
}
// the d openings of the polynomial at d_p (d Fr, device) -> d_proofs_aff: scalar half, the handle's transform, point half, in that order
keaki_status open_fk_from_poly(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_p, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                               const uint64_t* inv_2d, void* d_fr_work, void* d_g_work, void* d_proofs_aff) {
  FkPolyScalars s;
  ST_TRY(open_fk_poly_scalars_run(ctx, log2d, d_p, omega_2d, omega_2d_inv, inv_2d, d_fr_work, &s));
  ST_TRY(fk_cache_ensure(ctx, srs, log2d, s.tw));
  return open_fk_run(ctx, srs->fk.p, log2d, s.hat_a, s.tw, s.twi, d_g_work, d_proofs_aff);
}

// ---- host-pointer batches in CHUNKS ------------------------------------------------------------------------------------------
// A batch call that takes host arrays is upload -> kernels -> download; done in that order the device idles during both copies and the host
// thread during the kernels (vec_encrypt of 2^20 items: 8.1 ms per 2^18-item piece for 7.0 ms of kernels, profiles/r04_vec_encrypt_timeline.txt).
// Batches of two chunks or more run as a pipeline over two buffer halves: the upload of chunk k + 1 and the download of chunk k - 1 go
// through a copy stream of the context's own while the kernels of chunk k run on the context's stream. The host arrays are pageable, so a
// copy call returns when the runtime has staged (upload) or delivered (download) the bytes: one host thread is enough, and the order of its
// calls -- upload k, launch k, download k - 1 -- is what keeps the device busy. `up(lo, m, half, stream)` enqueues the uploads of items
// [lo, lo + m) into buffer half `half`, `run(lo, m, half)` the kernels (on ctx->stream), `down(lo, m, half, stream)` first-touches the
// caller's output pages and enqueues the downloads.
// chunk size of a batch of n items: `unit` items (PIPE_CHUNK: two rounds of the GT exponentiation kernel; the pairing path passes its own launch
// size -- 16 launches of 2^16 pairings take 3.6 ms longer than 8 of 2^17), the whole batch below two units
inline size_t pipe_chunk_items(const keaki_hip_ctx* ctx, size_t n, size_t unit = PIPE_CHUNK) { return ctx->tune.pipe_chunks && n >= 2 * unit ? unit : n; }
// `touch(lo, m)`: first-touch the caller's output ranges of items [lo, lo + m) (prefault_out). A download into pages that do not exist yet runs
// at 5 GB/s instead of 56 (bench_tools/ubench_pageable_copy_sizes.py), and touching them costs the host 40-125 us per MB: with one chunk that
// happens on the calling thread while the kernels run; with more, helper threads walk the chunks ahead of the downloads (one thread, three
// when the outputs exceed 64 MB: GT bytes out are 384 B per item) and a download waits for its chunk's flag, so no touch can land on delivered bytes.
template <class Up, class Run, class Touch, class Down>
static keaki_status pipelined(CopyFeed& feed, size_t n, size_t ch, size_t out_bytes_per_item, Up up, Run run, Touch touch, Down down) {
  keaki_hip_ctx* ctx = feed.ctx;
  ST_TRY(ctx->pipe.ready(ctx));
  feed.also_drain(ctx->pipe.copy_stream);       // an early exit leaves no copy of a chunk behind
  const size_t chunks = (n + ch - 1) / ch;
  hipStream_t cs = ctx->pipe.copy_stream, st = ctx->stream;
  const size_t n_helpers = chunks < 2 || !ctx->tune.host_prefault ? 0 : (n * out_bytes_per_item >= ((size_t)64 << 20) ? std::min<size_t>(3, chunks) : 1);
  std::unique_ptr<std::atomic<unsigned char>[]> touched(new std::atomic<unsigned char>[chunks]);
  for (size_t k = 0; k < chunks; k++) touched[k].store(0, std::memory_order_relaxed);
  // a helper touches (writes into) the output pages of chunk k only after chunk k's inputs have been read: a caller may pass one array as input
  // and output (messages in, bodies out). `staged` = chunks whose upload calls have returned (pageable: the source has been consumed by then);
  // `give_up` releases the helpers when the call leaves early.
  std::atomic<size_t> staged{0};
  std::atomic<bool> give_up{false};
  struct Helpers {
    std::vector<std::thread> t;
    std::atomic<bool>* give_up;
    ~Helpers() { give_up->store(true); for (auto& x : t) if (x.joinable()) x.join(); }
  } helpers{{}, &give_up};
  for (size_t h = 0; h < n_helpers; h++)
    helpers.t.emplace_back([&, h] {
      for (size_t k = h; k < chunks; k += n_helpers) {
        // yield first, not sleep: sleep_for(50 us) wakes late enough under load to cost a 2^20-item call 20 ms (measured: encap with GT out
        // 57 -> 73 ms). A wait that outlasts ~2 ms (the device is far behind: nothing to gain from a hot loop) falls back to short sleeps.
        for (unsigned spins = 0; staged.load(std::memory_order_acquire) <= k; spins++) {
          if (give_up.load(std::memory_order_relaxed)) return;
          if (spins < 20000) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        touch(k * ch, std::min(ch, n - k * ch));
        touched[k].store(1, std::memory_order_release);
      }
    });
  // the copy stream starts behind whatever the context's stream holds (an earlier call's kernels may still read the buffers)
  HIP_TRY(ctx, hipEventRecord(ctx->pipe.done[0], st));
  HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->pipe.done[0], 0));
  for (size_t k = 0; k <= chunks; k++) {
    if (k < chunks) {
      const size_t lo = k * ch, m = std::min(ch, n - lo);
      const int h = (int)(k & 1);
      ST_TRY(up(lo, m, h, cs));
      staged.store(k + 1, std::memory_order_release);
      HIP_TRY(ctx, hipEventRecord(ctx->pipe.in[h], cs));
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->pipe.in[h], 0));
      ST_TRY(run(lo, m, h));
      HIP_TRY(ctx, hipEventRecord(ctx->pipe.done[h], st));
    }
    if (k >= 1) {
      const size_t lo = (k - 1) * ch, m = std::min(ch, n - lo);
      const int h = (int)((k - 1) & 1);
      if (!n_helpers) touch(lo, m);
      else for (unsigned spins = 0; !touched[k - 1].load(std::memory_order_acquire); spins++) {
        if (spins < 20000) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->pipe.done[h], 0));
      ST_TRY(down(lo, m, h, cs));
    }
  }
  HIP_TRY(ctx, hipStreamSynchronize(cs));
  feed.settled();                               // every download of the call was behind its kernels on cs
  return KEAKI_OK;
}
// One per-item region of a pipelined host batch, `bytes` per item: `in` is uploaded into it, `out` downloaded from it (both: in place --
// messages in, bodies out), neither: device scratch.
struct Region { const void* in; void* out; size_t bytes; };
// A host batch through pipelined(): io_a = [head | half 0 | half 1], each half the chunk's regions one after the other (rounded to 256 B).
// The head -- constants of the whole batch, laid out like the regions of a single item -- goes up on ctx->stream before the chunks.
// `run(lo, m, d_head, d)` enqueues the kernels of items [lo, lo + m): d_head[i] = head region i, d[i] = region i of the chunk's half.
template <class Run>
static keaki_status pipelined_regions(keaki_hip_ctx* ctx, size_t n, size_t ch, std::initializer_list<Region> head,
                                      std::initializer_list<Region> regions, Run run) {
  const std::vector<Region> rg(regions);
  size_t head_bytes = 0, half = 0, out_bytes = 0;
  for (const Region& x : head) head_bytes += x.bytes;
  for (const Region& x : rg) { half += ch * x.bytes; if (x.out) out_bytes += x.bytes; }
  head_bytes = (head_bytes + 255) & ~(size_t)255;
  half = (half + 255) & ~(size_t)255;
  ST_TRY(reserve(ctx, ctx->io_a, head_bytes + 2 * half));
  std::vector<char*> d_head, d[2];
  char* p = (char*)ctx->io_a.p;
  CopyFeed feed(ctx);
  for (const Region& x : head) {
    d_head.push_back(p);
    ST_TRY(feed.put(0, p, x.in, x.bytes));
    p += x.bytes;
  }
  for (int h = 0; h < 2; h++) {
    p = (char*)ctx->io_a.p + head_bytes + h * half;
    for (const Region& x : rg) { d[h].push_back(p); p += ch * x.bytes; }
  }
  return pipelined(feed, n, ch, out_bytes,
    [&](size_t lo, size_t m, int h, hipStream_t cs) -> keaki_status {
      for (size_t i = 0; i < rg.size(); i++)
        if (rg[i].in) HIP_TRY(ctx, hipMemcpyAsync(d[h][i], (const char*)rg[i].in + lo * rg[i].bytes, m * rg[i].bytes, hipMemcpyHostToDevice, cs));
      return KEAKI_OK;
    },
    [&](size_t lo, size_t m, int h) -> keaki_status { return run(lo, m, d_head.data(), d[h].data()); },
    [&](size_t lo, size_t m) {
      for (const Region& x : rg) if (x.out) prefault_out(ctx, (char*)x.out + lo * x.bytes, m * x.bytes);
    },
    [&](size_t lo, size_t m, int h, hipStream_t cs) -> keaki_status {
      for (size_t i = 0; i < rg.size(); i++)
        if (rg[i].out) HIP_TRY(ctx, hipMemcpyAsync((char*)rg[i].out + lo * rg[i].bytes, d[h][i], m * rg[i].bytes, hipMemcpyDeviceToHost, cs));
      return KEAKI_OK;
    });
}


// ---- MSM of a scalar vector in HOST memory -----------------------------------------------------------------------------------------
// kzg::commit hands over a polynomial that lives in host memory (reference src/kzg.rs:89-101): the call is upload -> MSM, and done in
// that order the 512 MiB of a 2^24-term polynomial cost 11.5 ms of copy in front of 16.7 ms of kernels (BENCH_r04: 5.96e8/s against
// 1.007e9/s resident). From `msm_pipe_min` scalars on the vector goes up in point-range chunks through the copy stream and the MSM
// runs chunk by chunk behind it (msm_host.hip.h: MsmPipe): the upload of chunk j + 1 hides under the kernels of chunk j, only the
// first chunk's copy stays in front; `run(pipe)` enqueues the MSM over ctx->io_a.
// A pageable source makes every copy call return once its bytes are staged; a pinned one returns at once -- the order of the host's
// calls (copy j, kernels j, copy j + 1, ...) serves both.
// The chunk bounds: host_plan.h (msm_pipe_bounds). One piece is begin(false) and one put in front of the MSM.
template <class Run>
static keaki_status msm_from_host(CopyFeed& feed, const uint64_t* scalars, size_t n, Run run) {
  keaki_hip_ctx* ctx = feed.ctx;
  ST_TRY(reserve(ctx, ctx->io_a, n ? n * 32 : 16));
  MsmPipe pipe;
  const std::vector<size_t> bounds = msm_pipe_bounds(ctx->tune, n);
  for (size_t j = 0; j + 1 < bounds.size(); j++) pipe.ranges.push_back({bounds[j], bounds[j + 1] - bounds[j]});
  const bool chunked = pipe.ranges.size() >= 2;
  ST_TRY(feed.begin(chunked));
  pipe.stage = [&](size_t j) -> keaki_status {
    const size_t lo = pipe.ranges[j].first, m = pipe.ranges[j].second;
    return feed.put(j, (char*)ctx->io_a.p + lo * 32, (const char*)scalars + lo * 32, m * 32);
  };
  if (chunked) return run(&pipe);
  ST_TRY(pipe.stage(0));
  return run(nullptr);
}

// What tells the G1 and G2 forms of the SRS, MSM and mul_batch entries apart: the point sizes, the launchers and the names in messages and traces.
struct GroupEntries {
  size_t aff, jac;
  const char *srs, *precompute, *msm, *msm_trace, *mul, *mul_trace;
  decltype(&msm_g1_run) msm_run;
  decltype(&msm_g1_precompute_run) precompute_run;
  decltype(&g1_mul_batch_run) mul_run;
};
constexpr GroupEntries G1E = {G1_AFF_BYTES, G1_JAC_BYTES, "srs_g1", "srs_g1_precompute", "msm_g1", "keaki.msm_g1", "g1_mul_batch", "keaki.g1_mul_batch", msm_g1_run, msm_g1_precompute_run, g1_mul_batch_run};
constexpr GroupEntries G2E = {G2_AFF_BYTES, G2_JAC_BYTES, "srs_g2", "srs_g2_precompute", "msm_g2", "keaki.msm_g2", "g2_mul_batch", "keaki.g2_mul_batch", msm_g2_run, msm_g2_precompute_run, g2_mul_batch_run};
// ---- SRS handles: the eight keaki_hip_srs_g*_ entries forward here ----
template <class H>
keaki_status srs_upload(const GroupEntries& g, keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, H** out) {
  CTX_GUARD(ctx);
  if (!out || (n && !points_aff)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_upload: null pointer", g.srs);
  void* d = nullptr;
  HIP_TRY(ctx, hipMalloc(&d, n ? n * g.aff : 16));          // the caller's points: outside keaki_hip_debug_set_alloc_limit (internal.h: dev_alloc)
  if (n) {
    // on the context's stream (non-blocking: not ordered behind the null stream a plain hipMemcpy uses), complete before the call returns
    hipError_t e = hipMemcpyAsync(d, points_aff, n * g.aff, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); return fail(ctx, KEAKI_ERR_HIP, "srs upload copy failed: %s", hipGetErrorString(e)); }
  }
  *out = new_srs<H>(ctx, d, n, true);
  return KEAKI_OK;
}
template <class H>
keaki_status srs_wrap(const GroupEntries& g, keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, H** out) {
  CTX_GUARD(ctx);
  if (!out || (n && !d_points_aff)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_wrap_dev: null pointer", g.srs);
  *out = new_srs<H>(ctx, d_points_aff, n, false);
  return KEAKI_OK;
}
template <class H>
void srs_free(keaki_hip_ctx* ctx, H* srs) {
  if (!srs) return;
  if (ctx) { keaki_internal::DeviceScope dc_(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
  keaki_internal::DeviceScope dev_(srs->device);
  if (srs->owned && srs->d) (void)hipFree((void*)srs->d);
  if (srs->table) (void)hipFree(srs->table);
  size_t held = srs->table_bytes;          // booked on the context that built them, whichever context (or NULL) frees the handle
  srs->for_each_cache([&](SrsCache& c) { if (c.p) (void)hipFree(c.p); held += c.bytes; });
  with_live_ctx(srs->acct, [&](keaki_hip_ctx* a) { mem_sub(a->mem_tables, held); });
  delete srs;
}
template <class H>
keaki_status srs_precompute(const GroupEntries& g, keaki_hip_ctx* ctx, H* srs, size_t* table_bytes_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.srs_precompute");
  if (!srs) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: srs is null", g.precompute);
  SRS_CHECK(ctx, srs, g.precompute);
  std::lock_guard<std::recursive_mutex> hl(srs->mu);       // contexts sharing the handle: the first one builds, the others find the tables
  if (!srs->table && srs->n) {
    int c = 0; size_t bytes = 0; void* t = nullptr;
    ST_TRY(g.precompute_run(ctx, srs->d, srs->n, &c, &bytes, &t));
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(t); return fail(ctx, KEAKI_ERR_HIP, "%s: %s", g.precompute, hipGetErrorString(e)); }
    srs->c_table = c; srs->table_bytes = bytes; srs->table = t;       // published only when complete
    srs->acct = ctx; ctx->mem_tables += bytes;
  }
  if (table_bytes_out) *table_bytes_out = srs->table_bytes;
  return KEAKI_OK;
}
template <class Srs>
keaki_status msm_dev(const GroupEntries& g, keaki_hip_ctx* ctx, const Srs* srs, const void* d_scalars, size_t n, void* d_out_jac) {
  CTX_GUARD(ctx);
  TRACE_SCOPE(g.msm_trace);
  if (!srs) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: srs is null", g.msm);
  SRS_CHECK(ctx, srs, g.msm);
  const auto tb = srs_tables(srs);
  return g.msm_run(ctx, srs->d, srs->n, d_scalars, n, d_out_jac, tb.first, tb.second, nullptr);
}
template <class Srs>
keaki_status msm_host(const GroupEntries& g, keaki_hip_ctx* ctx, const Srs* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac) {
  CTX_GUARD(ctx);
  TRACE_SCOPE(g.msm_trace);
  if (!srs || !out_jac || (n && !scalars)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: null pointer", g.msm);
  ST_TRY(srs_holds(ctx, srs, g.msm, n, SRS_SHORT_MSM));
  ST_TRY(reserve(ctx, ctx->io_b, g.jac));
  const auto tb = srs_tables(srs);
  CopyFeed feed(ctx);
  ST_TRY(msm_from_host(feed, scalars, n, [&](const MsmPipe* pipe) {
    return g.msm_run(ctx, srs->d, srs->n, ctx->io_a.p, n, ctx->io_b.p, tb.first, tb.second, pipe);
  }));
  ST_TRY(download(feed, out_jac, ctx->io_b.p, g.jac));
  resolve_timing(ctx);
  return KEAKI_OK;
}
keaki_status mul_batch_dev(const GroupEntries& g, keaki_hip_ctx* ctx, const void* d_points_aff, int32_t point_stride, const void* d_scalars, size_t n, void* d_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE(g.mul_trace);
  if (n == 0) return KEAKI_OK;
  if (!d_points_aff || !d_scalars || !d_out_aff || (point_stride != 0 && point_stride != 1)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: bad argument", g.mul);
  return g.mul_run(ctx, d_points_aff, (int)point_stride, d_scalars, n, d_out_aff);
}
keaki_status mul_batch_host(const GroupEntries& g, keaki_hip_ctx* ctx, const uint64_t* points_aff, int32_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_aff) {
  CTX_GUARD(ctx);                 // held across stage -> kernel -> download: io_a/io_b/io_c belong to this call until it returns
  if (n == 0) return KEAKI_OK;
  if (!points_aff || !scalars || !out_aff || (point_stride != 0 && point_stride != 1)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: bad argument", g.mul);
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, points_aff, (point_stride ? n : 1) * g.aff));
  ST_TRY(upload(feed, ctx->io_b, scalars, n * 32));
  ST_TRY(reserve(ctx, ctx->io_c, n * g.aff));
  ST_TRY(mul_batch_dev(g, ctx, ctx->io_a.p, point_stride, ctx->io_b.p, n, ctx->io_c.p));
  prefault_out(ctx, out_aff, n * g.aff);
  return download(feed, out_aff, ctx->io_c.p, n * g.aff);
}

}  // namespace


#ifndef KEAKI_SRC_HASH
#define KEAKI_SRC_HASH "unknown"
#endif
// "... src=<hash>": the hash of the kernel sources this binary was built from (csrc/Makefile, bench_tools/srchash.py); the profile
// collectors stamp their output with it and bench.py refuses figures measured on another build.
#ifdef KEAKI_DIAG
const char* keaki_hip_version(void) { return "keaki-hip 0.3 (gfx950) DIAGNOSTIC BUILD (diag_row_mask available: not the product) src=" KEAKI_SRC_HASH; }
#else
const char* keaki_hip_version(void) { return "keaki-hip 0.3 (gfx950) src=" KEAKI_SRC_HASH; }
#endif

namespace {
// The tuning options (Tuning, internal.h), each declared ONCE: keaki_hip_ctx_set_option and the environment (tune_from_env) both go through
// this table. An option is named after its member, its variable is KEAKI_<NAME>, and its value converts as the member's type does ((int)v,
// v != 0, long long). `refuses(ctx, name, v)`: the values set_option fails (KEAKI_ERR_BAD_ARG, the message recorded on ctx); the environment
// asks with ctx = nullptr and ignores what is refused. `on_change`: what a set_option that changes the value invalidates.
struct TuneOption {
  const char* name;
  bool (*assign)(Tuning& t, long long v);                               // true: the value changed
  bool (*refuses)(keaki_hip_ctx* ctx, const char* name, long long v) = nullptr;
  void (*on_change)(keaki_hip_ctx* ctx) = nullptr;
  bool from_env = true;
};
template <auto M>
bool assign_member(Tuning& t, long long v) {
  auto& f = t.*M;
  const auto old = f;
  f = (std::remove_reference_t<decltype(f)>)v;
  return f != old;
}
template <int MX>
bool msm_c_refuses(keaki_hip_ctx* ctx, const char* name, long long v) {           // a width no plan can run (the environment: stays automatic)
  if (!msm_c_too_wide(v, MX)) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: %s = %lld exceeds %d, the widest window whose buckets the bucket sort can address (3 .. %d; 0 = automatic)",
                name, v, MX, MX);
  return true;
}
bool gt_wb_b_refuses(keaki_hip_ctx* ctx, const char*, long long v) {          // the environment's width is taken as it is: b_table refuses it on use
  if (!ctx || v == 0 || (v >= 8 && v <= 22 && gt_table_powers((uint32_t)v) <= 320)) return false;
  fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: gt_wb_b = %lld out of range", v);
  return true;
}
bool fk_coset_group_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v == 0 || v == 1 || v == 2 || v == 4) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: fk_coset_group = %lld must be 1, 2 or 4 (0 = %u)", v, FKC_G);
  return true;
}
bool fk_coset_min_lanes_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= ((long long)1 << 31)) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: fk_coset_min_lanes = %lld out of range (1 .. 2^31; 0 = %u)", v, FKC_SPLIT_MIN_LANES);
  return true;
}
bool vec_update_k_pass_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= (long long)UPD_K_PASS) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: vec_update_k_pass = %lld out of range (1 .. %u; 0 = %u)", v, UPD_K_PASS, UPD_K_PASS);
  return true;
}
bool verify_cosets_blocks_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= (long long)VC_MAX_BLOCKS) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: verify_cosets_blocks = %lld out of range (1 .. %u; 0 = automatic)", v, VC_MAX_BLOCKS);
  return true;
}
bool verify_sets_blocks_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= (long long)VS_MAX_BLOCKS) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: verify_sets_blocks = %lld out of range (1 .. %u; 0 = automatic)", v, VS_MAX_BLOCKS);
  return true;
}
bool coset_rows_min_lanes_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= ((long long)1 << 31)) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: coset_rows_min_lanes = %lld out of range (1 .. 2^31; 0 = %u)", v, CR_MIN_LANES);
  return true;
}
bool coset_rows_route_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= 2) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: coset_rows_route = %lld must be 0 (by plan), 1 (window table) or 2 (batched MSM)", v);
  return true;
}
bool coset_rows_wb_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v == 0 || v == 8 || v == 10 || v == 13) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: coset_rows_wb = %lld must be 8, 10 or 13 (0 = by plan)", v);
  return true;
}
bool set_rows_wb_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v == 0 || v == 8 || v == 10 || v == 13) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: set_rows_wb = %lld must be 8, 10 or 13 (0 = by plan)", v);
  return true;
}
bool set_rows_min_lanes_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= ((long long)1 << 31)) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: set_rows_min_lanes = %lld out of range (1 .. 2^31; 0 = %u)", v, SR_MIN_LANES);
  return true;
}
bool set_each_route_refuses(keaki_hip_ctx* ctx, const char*, long long v) {
  if (v >= 0 && v <= 2) return false;
  if (ctx) fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: set_each_route = %lld must be 0 (by plan), 1 (the fused pairing kernel) or 2 (two Miller loops per item)", v);
  return true;
}
#define TUNE_OPTION(member, ...) TuneOption{#member, assign_member<&Tuning::member>, __VA_ARGS__}
const TuneOption TUNE_OPTIONS[] = {
    TUNE_OPTION(msm_c, msm_c_refuses<MSM_C_MAX>), TUNE_OPTION(msm_c_shared, msm_c_refuses<MSM_C_SHARED_MAX>), TUNE_OPTION(msm_short_tables),
    TUNE_OPTION(reduce_l), TUNE_OPTION(part_shift), TUNE_OPTION(acc_u29), TUNE_OPTION(acc_u29_g2), TUNE_OPTION(acc_prefetch), TUNE_OPTION(acc_idxq),
    TUNE_OPTION(cs_masked), TUNE_OPTION(acc_nt), TUNE_OPTION(fk_uniform), TUNE_OPTION(fk_gtab), TUNE_OPTION(fk_radix4), TUNE_OPTION(fk_addsub29),
    TUNE_OPTION(fb_occ1), TUNE_OPTION(pair_wide_max), TUNE_OPTION(pair_two_waves),
    TUNE_OPTION(gt_wb_b, gt_wb_b_refuses, [](keaki_hip_ctx* ctx) { ctx->kem.gt_b_ready = ctx->kem.gt_b_fallback = false; }),   // B's table: rebuilt at the new width on next use
    TUNE_OPTION(encap_gt), TUNE_OPTION(encap_multi_single_min), TUNE_OPTION(host_prefault), TUNE_OPTION(pipe_chunks), TUNE_OPTION(msm_pipe_chunks), TUNE_OPTION(msm_pipe_min),
    TUNE_OPTION(msm_pipe_growth), TUNE_OPTION(vec_update_k_pass, vec_update_k_pass_refuses),
    TUNE_OPTION(fk_coset_group, fk_coset_group_refuses), TUNE_OPTION(fk_coset_min_lanes, fk_coset_min_lanes_refuses),
    TUNE_OPTION(verify_cosets_blocks, verify_cosets_blocks_refuses), TUNE_OPTION(verify_sets_blocks, verify_sets_blocks_refuses),
    TUNE_OPTION(coset_rows_min_lanes, coset_rows_min_lanes_refuses), TUNE_OPTION(coset_rows_route, coset_rows_route_refuses),
    TUNE_OPTION(coset_rows_wb, coset_rows_wb_refuses),
    TUNE_OPTION(set_rows_wb, set_rows_wb_refuses), TUNE_OPTION(set_rows_min_lanes, set_rows_min_lanes_refuses), TUNE_OPTION(set_each_route, set_each_route_refuses),
#ifdef KEAKI_DIAG
    TUNE_OPTION(diag_row_mask, nullptr, nullptr, false),       // set_option only: no environment variable
#endif
};
#undef TUNE_OPTION
// The ONE place the library reads the environment: initial values of a context's tuning switches (an unset or empty variable is ignored).
void tune_from_env(Tuning& t) {
  for (const TuneOption& o : TUNE_OPTIONS) {
    if (!o.from_env) continue;
    std::string var = "KEAKI_";
    for (const char* c = o.name; *c; c++) var += (char)toupper((unsigned char)*c);
    const char* e = getenv(var.c_str());
    if (!e || !*e) continue;
    const long long v = atoll(e);
    if (!o.refuses || !o.refuses(nullptr, o.name, v)) o.assign(t, v);
  }
}
struct BufClass { DevBuf* b; int cls; };   // cls: 1 = workspace, 2 = GT / fixed-base tables of encapsulate
std::vector<BufClass> all_bufs(keaki_hip_ctx* ctx) {      // the list is keaki_hip_ctx::for_each_buf (internal.h), beside the declarations
  std::vector<BufClass> v;
  ctx->for_each_buf([&](DevBuf* b, int cls) { v.push_back({b, cls}); });
  return v;
}
}  // namespace

keaki_status keaki_hip_ctx_create(int32_t device, void* stream, keaki_hip_ctx** out) {
  if (!out) return fail(nullptr, KEAKI_ERR_BAD_ARG, "ctx_create: out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, KEAKI_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(nullptr, KEAKI_ERR_BAD_ARG, "device %d out of range (%d visible)", device, ndev);
  keaki_internal::DeviceScope dev_(device);
  if (!dev_.ok) return fail(nullptr, KEAKI_ERR_HIP, "hipSetDevice(%d) failed", device);
  hipDeviceProp_t prop;
  HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, KEAKI_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
  keaki_hip_ctx* ctx = new keaki_hip_ctx();
  ctx->device = device;
  ctx->n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
  tune_from_env(ctx->tune);
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return fail(nullptr, KEAKI_ERR_HIP, "hipStreamCreate failed");
    }
    ctx->own_stream = true;
  }
  for (auto& e : ctx->ev) (void)hipEventCreate(&e);
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live_ctx.insert(ctx); }
  *out = ctx;
  return KEAKI_OK;
}

void keaki_hip_ctx_destroy(keaki_hip_ctx* ctx) {
  if (!ctx) return;
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live_ctx.erase(ctx); }
  {
  keaki_internal::DeviceScope dev_(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (const BufClass& bc : all_bufs(ctx))
    if (bc.b->p) (void)hipFree(bc.b->p);
  for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->fk_ev) if (e) (void)hipEventDestroy(e);
  ctx->pipe.destroy();
  ctx->aux.destroy();
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
}

// The message is copied under the context lock into a buffer of the CALLING thread (valid until that thread's next call of this
// function), so a concurrent failing call on another thread cannot reallocate the string under the reader.
const char* keaki_hip_last_error(const keaki_hip_ctx* ctx) {
  if (!ctx) return g_create_error.c_str();
  thread_local std::string copy;
  keaki_hip_ctx* c = const_cast<keaki_hip_ctx*>(ctx);
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  copy = c->err;
  return copy.c_str();
}

keaki_status keaki_hip_ctx_set_option(keaki_hip_ctx* ctx, const char* name, int64_t value) {
  if (!ctx) return KEAKI_ERR_BAD_ARG;
  std::lock_guard<std::recursive_mutex> lock_(ctx->mu);
  if (!name) return fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: name is null");
  for (const TuneOption& o : TUNE_OPTIONS) {
    if (strcmp(o.name, name) != 0) continue;
    if (o.refuses && o.refuses(ctx, name, value)) return KEAKI_ERR_BAD_ARG;
    if (o.assign(ctx->tune, value) && o.on_change) o.on_change(ctx);
    return KEAKI_OK;
  }
  return fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_set_option: unknown option '%s'", name);
}
keaki_status keaki_hip_debug_set_alloc_limit(keaki_hip_ctx* ctx, size_t bytes) {
  if (!ctx) return KEAKI_ERR_BAD_ARG;
  std::lock_guard<std::recursive_mutex> lock_(ctx->mu);
  ctx->tune.alloc_limit = bytes;
  return KEAKI_OK;
}
// Test hook: every byte of every scratch workspace (keaki_hip_ctx::for_each_scratch) becomes `byte`, the full capacity, behind everything the context's
// three streams hold; with also_new the allocation gate fills what it hands out from then on. The caches of KemState and the tables of SRS handles stay.
keaki_status keaki_hip_debug_poison_workspaces(keaki_hip_ctx* ctx, uint32_t byte, int32_t also_new) {
  CTX_GUARD(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->aux.stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->aux.stream));
  if (ctx->pipe.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe.copy_stream));
  hipError_t e = hipSuccess;
  ctx->for_each_scratch([&](DevBuf* b, int) {
    if (b->p && b->cap && e == hipSuccess) e = hipMemsetAsync(b->p, (int)(byte & 0xff), b->cap, ctx->stream);
  });
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->poison_new = also_new ? (int)(byte & 0xff) : -1;
  return KEAKI_OK;
}
// Releases every grow-only workspace and encapsulate table of the context (they come back on the next call that needs them; a table's
// rebuild costs what the first call cost). SRS handles are not touched.
keaki_status keaki_hip_ctx_trim(keaki_hip_ctx* ctx) {
  CTX_GUARD(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->aux.stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->aux.stream));      // a table build a failed call left behind
  if (ctx->pipe.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe.copy_stream));
  for (const BufClass& bc : all_bufs(ctx))
    if (bc.b->p) { (void)hipFree(bc.b->p); bc.b->p = nullptr; bc.b->cap = 0; }
  ctx->kem = KemState();         // the buffers are gone: no ready or valid bit outlives its table
  return KEAKI_OK;
}
keaki_status keaki_hip_ctx_memory(keaki_hip_ctx* ctx, size_t* out4) {
  if (!ctx) return KEAKI_ERR_BAD_ARG;
  std::lock_guard<std::recursive_mutex> lock_(ctx->mu);
  if (!out4) return fail(ctx, KEAKI_ERR_BAD_ARG, "ctx_memory: out4 is null");
  size_t ws = 0, gt = 0;
  for (const BufClass& bc : all_bufs(ctx)) (bc.cls == 1 ? ws : gt) += bc.b->cap;
  out4[0] = ctx->mem_tables; out4[1] = ws; out4[2] = gt; out4[3] = ctx->mem_tables + ws + gt;
  return KEAKI_OK;
}

void* keaki_hip_ctx_stream(const keaki_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int32_t keaki_hip_ctx_device(const keaki_hip_ctx* ctx) { return ctx ? ctx->device : -1; }

keaki_status keaki_hip_synchronize(keaki_hip_ctx* ctx) {
  CTX_GUARD(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  resolve_timing(ctx);
  return KEAKI_OK;
}

keaki_status keaki_hip_set_timing(keaki_hip_ctx* ctx, int32_t enabled) {
  CTX_GUARD(ctx);
  ctx->timing = enabled != 0;
  if (ctx->timing && !ctx->fk_ev[0])
    for (auto& e : ctx->fk_ev) (void)hipEventCreate(&e);
  return KEAKI_OK;
}
// device time of the last FK23 call (keaki_hip_open_fk[_poly]) with timing enabled, milliseconds: out3 = [the 2d pointwise scalar-mults,
// the butterfly stages of the two size-d transforms (k_g1_fft_stage_map + the twist), the whole device pipeline]; < 0 if none
keaki_status keaki_hip_last_fk_ms(keaki_hip_ctx* ctx, float* out3) {
  CTX_GUARD(ctx);
  if (!out3) return fail(ctx, KEAKI_ERR_BAD_ARG, "last_fk_ms: out3 is null");
  resolve_fk_timing(ctx);
  for (int i = 0; i < 3; i++) out3[i] = ctx->last_fk_ms[i];
  return KEAKI_OK;
}
float keaki_hip_last_msm_bucket_ms(const keaki_hip_ctx* ctx) { return ctx ? ctx->last_bucket_ms : -1.f; }
float keaki_hip_last_msm_total_ms(const keaki_hip_ctx* ctx) { return ctx ? ctx->last_total_ms : -1.f; }
int32_t keaki_hip_last_msm_window_bits(const keaki_hip_ctx* ctx) { return ctx ? ctx->last_c : 0; }

// ---- SRS -----------------------------------------------------------------------------------------
keaki_status keaki_hip_srs_g1_upload(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, keaki_hip_srs_g1** out) { return srs_upload(G1E, ctx, points_aff, n, out); }
keaki_status keaki_hip_srs_g2_upload(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, keaki_hip_srs_g2** out) { return srs_upload(G2E, ctx, points_aff, n, out); }
keaki_status keaki_hip_srs_g1_wrap_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, keaki_hip_srs_g1** out) { return srs_wrap(G1E, ctx, d_points_aff, n, out); }
keaki_status keaki_hip_srs_g2_wrap_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, keaki_hip_srs_g2** out) { return srs_wrap(G2E, ctx, d_points_aff, n, out); }
void keaki_hip_srs_g1_free(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs) { srs_free(ctx, srs); }
void keaki_hip_srs_g2_free(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs) { srs_free(ctx, srs); }
keaki_status keaki_hip_srs_g1_precompute(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, size_t* table_bytes_out) { return srs_precompute(G1E, ctx, srs, table_bytes_out); }
keaki_status keaki_hip_srs_g2_precompute(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs, size_t* table_bytes_out) { return srs_precompute(G2E, ctx, srs, table_bytes_out); }
// non-owning view of points [offset, offset + n) of an uploaded SRS: the chunk a rank owns when an MSM is sharded by point range
keaki_status keaki_hip_srs_g1_slice(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, size_t offset, size_t n, keaki_hip_srs_g1** out) {
  CTX_GUARD(ctx);
  if (!srs || !out) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g1_slice: null pointer");
  if (offset > srs->n || n > srs->n - offset) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g1_slice: [%zu, %zu) is outside the %zu points of the SRS", offset, offset + n, srs->n);
  if (srs->device != ctx->device) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g1_slice: the SRS lives on device %d, this context on device %d", srs->device, ctx->device);
  *out = new_srs<keaki_hip_srs_g1>(ctx, (const char*)srs->d + offset * G1_AFF_BYTES, n, false);
  return KEAKI_OK;
}
size_t keaki_hip_srs_g1_len(const keaki_hip_srs_g1* srs) { return srs ? srs->n : 0; }

// ---- MSM -----------------------------------------------------------------------------------------
keaki_status keaki_hip_msm_g1_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_scalars, size_t n, void* d_out_jac) {
  return msm_dev(G1E, ctx, srs, d_scalars, n, d_out_jac);
}
keaki_status keaki_hip_msm_g1(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac) {
  return msm_host(G1E, ctx, srs, scalars, n, out_jac);
}
keaki_status keaki_hip_msm_g2_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g2* srs, const void* d_scalars, size_t n, void* d_out_jac) {
  return msm_dev(G2E, ctx, srs, d_scalars, n, d_out_jac);
}
keaki_status keaki_hip_msm_g2(keaki_hip_ctx* ctx, const keaki_hip_srs_g2* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac) {
  return msm_host(G2E, ctx, srs, scalars, n, out_jac);
}
keaki_status keaki_hip_g1_sum_dev(keaki_hip_ctx* ctx, const void* d_points_jac, size_t k, void* d_out_jac) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.g1_sum");
  if (!d_out_jac || (k && !d_points_jac)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g1_sum: null pointer");
  return g1_sum_run(ctx, d_points_jac, k, d_out_jac);
}
keaki_status keaki_hip_g1_sum(keaki_hip_ctx* ctx, const uint64_t* points_jac, size_t k, uint64_t* out_jac) {
  CTX_GUARD(ctx);
  if (!out_jac || (k && !points_jac)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g1_sum: null pointer");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, points_jac, k * 96));
  ST_TRY(reserve(ctx, ctx->io_b, 96));
  ST_TRY(g1_sum_run(ctx, ctx->io_a.p, k, ctx->io_b.p));
  return download(feed, out_jac, ctx->io_b.p, 96);
}

// ---- batched scalar multiplication -------------------------------------------------------------------
keaki_status keaki_hip_g1_mul_batch_dev(keaki_hip_ctx* ctx, const void* d_points_aff, int32_t point_stride, const void* d_scalars, size_t n, void* d_out_aff) {
  return mul_batch_dev(G1E, ctx, d_points_aff, point_stride, d_scalars, n, d_out_aff);
}
keaki_status keaki_hip_g2_mul_batch_dev(keaki_hip_ctx* ctx, const void* d_points_aff, int32_t point_stride, const void* d_scalars, size_t n, void* d_out_aff) {
  return mul_batch_dev(G2E, ctx, d_points_aff, point_stride, d_scalars, n, d_out_aff);
}
keaki_status keaki_hip_g1_mul_batch(keaki_hip_ctx* ctx, const uint64_t* points_aff, int32_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_aff) {
  return mul_batch_host(G1E, ctx, points_aff, point_stride, scalars, n, out_aff);
}
keaki_status keaki_hip_g2_mul_batch(keaki_hip_ctx* ctx, const uint64_t* points_aff, int32_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_aff) {
  return mul_batch_host(G2E, ctx, points_aff, point_stride, scalars, n, out_aff);
}

// ---- pairing ---------------------------------------------------------------------------------------------
keaki_status keaki_hip_pairing_batch_dev(keaki_hip_ctx* ctx, const void* d_g1_aff, const void* d_g2_aff, int32_t g2_stride, size_t n,
                                         void* d_gt_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.pairing");
  if (n == 0) return KEAKI_OK;
  if (!d_g1_aff || !d_g2_aff || !d_gt_out || (g2_stride != 0 && g2_stride != 1)) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing_batch: bad argument");
  return pairing_run(ctx, d_g1_aff, d_g2_aff, (int)g2_stride, n, d_gt_out);
}
keaki_status keaki_hip_pairing_batch(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, int32_t g2_stride, size_t n,
                                     uint8_t* gt_out) {
  CTX_GUARD(ctx);
  if (n == 0) return KEAKI_OK;
  if (!g1_aff || !g2_aff || !gt_out || (g2_stride != 0 && g2_stride != 1)) return fail(ctx, KEAKI_ERR_BAD_ARG, "pairing_batch: bad argument");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, g1_aff, n * 64));
  ST_TRY(upload(feed, ctx->io_b, g2_aff, (g2_stride ? n : 1) * 128));
  ST_TRY(reserve(ctx, ctx->io_c, n * 384));
  ST_TRY(keaki_hip_pairing_batch_dev(ctx, ctx->io_a.p, ctx->io_b.p, g2_stride, n, ctx->io_c.p));
  prefault_out(ctx, gt_out, n * 384);
  return download(feed, gt_out, ctx->io_c.p, n * 384);
}

// the context's second stream (internal.h: AuxLane) is for work that is bound by latency, not by the device; this is the means to
// send the launchers -- which all enqueue on ctx->stream -- there for a scope (the caller holds the context lock)
struct StreamSwap {
  keaki_hip_ctx* ctx;
  hipStream_t saved;
  StreamSwap(keaki_hip_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
  ~StreamSwap() { ctx->stream = saved; }
};
// signed-window table of e(P, g2) for a G1 point P in device memory: the powers of two e(P, g2)^(2^s) = e(P, 2^s g2) come from ONE pairing
// launch of P against the tabulated line sequences of the multiples 2^s g2 (the latency of one pairing; the tables -- 320 x 18 KB -- are built
// once per context: lane s doubles g2 s times, one k_g2_prepare workgroup per multiple), not from 260 doublings of P one after the other (1.4 ms).
constexpr uint32_t GT_POWERS_MAX = 320;
static keaki_status g2pow_tables(keaki_hip_ctx* ctx) {
  KemState& k = ctx->kem;
  if (k.g2pow_ready) return KEAKI_OK;
  ST_TRY(reserve(ctx, k.g2pow_lines, (size_t)GT_POWERS_MAX * g2_prepared_bytes()));
  ST_TRY(reserve(ctx, k.g2pow_pts, (size_t)(GT_POWERS_MAX + 1) * G2_AFF_BYTES));
  char* gen = (char*)k.g2pow_pts.p;
  char* pts = gen + G2_AFF_BYTES;
  ST_TRY(g2_generator_to(ctx, gen));
  ST_TRY(g2_pow2_multiples_run(ctx, gen, GT_POWERS_MAX, pts));
  ST_TRY(g2_prepare_run(ctx, pts, k.g2pow_lines.p, GT_POWERS_MAX));
  k.g2pow_ready = true;
  return KEAKI_OK;
}
static keaki_status gt_table_of(keaki_hip_ctx* ctx, const void* d_p_aff, void* d_table, uint32_t wb) {
  char* gb = (char*)ctx->kem.gt_base.p;
  const uint32_t cnt = gt_table_powers(wb);
  if (cnt > GT_POWERS_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "gt_table_of: %u powers", cnt);
  void* pows = gb + G1_AFF_BYTES + 320 * G1_AFF_BYTES;
  ST_TRY(g2pow_tables(ctx));
  ST_TRY(pairing_raw_fixed_run(ctx, d_p_aff, 0, cnt, ctx->kem.g2pow_lines.p, g2_prepared_lines(), pows));
  return gt_table_run(ctx, pows, d_table, wb);
}

// ---- KEM composites ------------------------------------------------------------------------------------------
// what a host-pointer entry point knows without asking the device: the two constants of the batch (no read-back, no stream synchronisation
// between the upload and the kernels), the size of the WHOLE batch this chunk belongs to, and whether it is its first chunk
struct EncapHost { const uint64_t* com; const uint64_t* tau; size_t n_batch; bool first; };
struct EncapArgs {
  const void *d_com, *d_tau, *d_points, *d_values, *d_r;   // device inputs: the commitment, [tau]_2 | n x 32 B each
  void *d_ct_out, *d_gt_out, *d_key_out;                   // n x 128 B | n x 384 B or null | n x msg_len B or null
  size_t n, msg_len;
  bool xor_into = false;                                   // the KDF XORs the key into d_key_out in place (the DEM)
  const EncapHost* host = nullptr;
};
// the fixed-base tables (window widths: api_host.h, FB_WB_*): batches below FB_TABLES_MIN items use the small 8-bit tables
constexpr uint32_t FB_TABLES_MIN = 256;
// window widths of the GT tables. The constant B = e(g1, g2) is tabulated once per context: 20-bit windows (13 products per item, 2.6 GB; option
// gt_wb_b picks another width). A = e(C, g2) per commitment: 13 bits on first sight (20 products per item, 31.5 MB: one launch of the twelve-lane pairing
// kernel over the tabulated multiples of g2 + the fills, 1.7 ms); when it comes back, 16 bits (201 MB) from the powers still lying in gt_base (0.5 ms).
constexpr uint32_t GT_WB_A_FIRST = 13, GT_WB_A_REPEAT = 16;
// The batch policy (no HIP call) from the size of the WHOLE batch, Tuning::gt_wb_b and encap_gt, the consecutive calls that carried this commitment, whether
// its A table is cached, and `prep` (keaki_hip_encap_prepare: no commitment). ALL calls take the GT path since the table of a new commitment costs 1.7 ms
// beside the ciphertext kernel: ~30 Fq12 products per item instead of two G1 ladders and a pairing. Option encap_gt = N keeps the per-item pairing below
// N items for a commitment without a table. B: 20-bit windows for batches of >= 65,536 items, else 16 (201 MB); widened once when a large batch comes
struct EncapPolicy { bool use_tables, use_gt; uint32_t wb_b_req; };
static EncapPolicy encap_policy(size_t n_policy, int gt_wb_b, long long encap_gt, uint32_t seen_com_runs, bool a_cached, bool prep) {
  const bool gt_env = encap_gt >= 0;
  const bool use_gt = n_policy >= (gt_env ? (size_t)encap_gt : (size_t)0) || (!prep && !gt_env && (a_cached || seen_com_runs >= 3));
  return {n_policy >= FB_TABLES_MIN, use_gt, gt_wb_b != 0 ? (uint32_t)gt_wb_b : (n_policy >= 65536 ? 20u : 16u)};
}
static void note_commitment(KemState& k, const uint64_t* com_host, bool first_of_batch) {   // consecutive calls with one commitment (a host batch's chunks are ONE call)
  const bool same = k.seen_com_runs && memcmp(com_host, k.seen_com, 64) == 0;
  if (same && first_of_batch && k.seen_com_runs < 1000000) k.seen_com_runs++;
  if (!same) { memcpy(k.seen_com, com_host, 64); k.seen_com_runs = 1; }
}
// the table of a new commitment is built on the aux stream; `gt_a_pending_aux` says that the context's stream has not been made to wait for that build yet. It survives
// an early error return, so a later call that finds the table published or rewrites gt_base orders itself behind the build first -- whatever happened in between.
static keaki_status wait_aux(keaki_hip_ctx* ctx) {
  if (ctx->kem.gt_a_pending_aux) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux.ev[1], 0));
  ctx->kem.gt_a_pending_aux = false;
  return KEAKI_OK;
}
static keaki_status b_table(keaki_hip_ctx* ctx, uint32_t wb_b_req) {      // GT path, the part of the setup: gt_base and the table of B at (at least) this width
  KemState& k = ctx->kem;
  ST_TRY(wait_aux(ctx));                                   // a build an earlier (failed) call left unawaited
  ST_TRY(reserve(ctx, k.gt_base, G1_AFF_BYTES + 320 * (G1_AFF_BYTES + 384)));   // a point | (unused since round 4) | the powers' pairings
  if (k.gt_b_ready && (ctx->tune.gt_wb_b != 0 || wb_b_req <= k.gt_b_wb || k.gt_b_fallback)) return KEAKI_OK;   // a forced width is never widened
  if (wb_b_req < 8 || wb_b_req > 22 || gt_table_powers(wb_b_req) > 320) return fail(ctx, KEAKI_ERR_BAD_ARG, "gt_wb_b = %u out of range", wb_b_req);
  k.gt_b_ready = false; k.gt_b_wb = wb_b_req;
  keaki_status st_b = reserve(ctx, k.gt_tab_b, gt_table_bytes(k.gt_b_wb));
  if (st_b == KEAKI_ERR_OOM && k.gt_b_wb > 16) {           // no room for the wide table: the 16-bit one is 201 MB
    (void)hipGetLastError();
    k.gt_b_wb = 16; k.gt_b_fallback = true;
    st_b = reserve(ctx, k.gt_tab_b, gt_table_bytes(k.gt_b_wb));
  }
  ST_TRY(st_b);
  ST_TRY(g1_generator_to(ctx, k.gt_base.p));
  ST_TRY(gt_table_of(ctx, k.gt_base.p, k.gt_tab_b.p, k.gt_b_wb));
  k.gt_b_ready = true;
  k.gt_a.invalidate();                                     // gt_base now holds B's powers
  return KEAKI_OK;
}
// GT path, the part of the commitment: A is reused while the caller keeps encrypting to the same commitment. A NEW commitment's table is a latency-bound
// job (65 waves for 1.4 ms, then the fills): it goes to a stream of its own, IN FRONT of the ciphertext kernel, which fills the device for 0.56 ms at
// 2^16 items -- the two run side by side and the exponentiation waits for both.
struct AuxBuild { bool a_on_aux = false, b_factor_done = false; };
static keaki_status a_table(keaki_hip_ctx* ctx, const EncapArgs& a, const uint64_t* com_host, bool first_of_batch, AuxBuild* out) {
  KemState& k = ctx->kem;
  if (!k.gt_a.holds(com_host)) {
    k.gt_a.invalidate();
    ST_TRY(reserve(ctx, k.gt_a.buf, gt_table_bytes(GT_WB_A_REPEAT)));
    ST_TRY(ctx->aux.ready(ctx));
    HIP_TRY(ctx, hipEventRecord(ctx->aux.ev[0], ctx->stream));          // behind every earlier reader of the table and of gt_base
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux.stream, ctx->aux.ev[0], 0));
    { StreamSwap on_aux(ctx, ctx->aux.stream); ST_TRY(gt_table_of(ctx, a.d_com, k.gt_a.buf.p, GT_WB_A_FIRST)); }
    HIP_TRY(ctx, hipEventRecord(ctx->aux.ev[1], ctx->aux.stream));
    k.gt_a_pending_aux = out->a_on_aux = true;
    if (a.n > 4096) {
      // the constant base's factor FIRST on the main stream: it fills every SIMD (two waves of 256 registers each) and must be out of the way
      // when the table's fill levels arrive; the ciphertext kernel behind it leaves half of each SIMD's registers to them
      ST_TRY(reserve(ctx, ctx->tmp_a, a.n * 384));
      ST_TRY(gt_encap_exp_run(ctx, nullptr, 0, k.gt_tab_b.p, k.gt_b_wb, a.d_values, a.d_r, a.n, nullptr, nullptr, ctx->tmp_a.p));
      out->b_factor_done = true;
    }
    k.gt_a.publish(com_host, GT_WB_A_FIRST);
  } else if (first_of_batch && k.gt_a.wb != GT_WB_A_REPEAT) {
    // same commitment again IN A LATER CALL (the chunks of one host batch keep their first chunk's table): the 260 powers of the first build cover the 256 needed
    ST_TRY(gt_table_run(ctx, (char*)k.gt_base.p + G1_AFF_BYTES + 320 * G1_AFF_BYTES, k.gt_a.buf.p, GT_WB_A_REPEAT));
    k.gt_a.wb = GT_WB_A_REPEAT;
  }
  return KEAKI_OK;
}
// The tables behind the ciphertexts ct_i = r_i [tau]_2 - (r_i alpha_i) g2, two fixed-base sums. [tau]_2 belongs to the setup, not to the batch: its window
// table is rebuilt only when the point changes. Batches of >= FB_TABLES_MIN items use (and build) the 16-bit tables; smaller ones use them when they hold
// this [tau]_2, else SMALL 8-bit tables (32 x 129 entries per base, 0.5 MB, built in the latency of one G2 scalar-mult): 64 mixed additions per item
// instead of two 254-step ladders (a single `encapsulate` call: 20.5 -> 10 ms). Afterwards the big table holds this [tau]_2, or else the small one does.
static keaki_status tau_table(keaki_hip_ctx* ctx, bool use_tables, const void* d_tau, const uint64_t* tau_host) {
  KemState& k = ctx->kem;
  const bool big = use_tables || (k.fb_ready && k.fb_tau.holds(tau_host));
  if (!big) ST_TRY(small_g2_tables(ctx, ctx->tmp_c.p));
  KeyedTable<16>& t = big ? k.fb_tau : k.fbs_tau;
  if (t.holds(tau_host)) return KEAKI_OK;
  t.invalidate();
  ST_TRY(g2_fb_table_run(ctx, d_tau, t.buf.p, big ? FB_WB_LONG : FB_WB_SMALL));
  t.publish(tau_host, big ? FB_WB_LONG : FB_WB_SMALL);
  return KEAKI_OK;
}
static keaki_status kem_setup(keaki_hip_ctx* ctx, const void* d_tau, size_t n_policy) {    // what depends on the SETUP only: nothing per item or commitment
  const EncapPolicy pol = encap_policy(n_policy, ctx->tune.gt_wb_b, ctx->tune.encap_gt, 0, false, true);
  ST_TRY(generator_tables(ctx, pol.use_tables));
  uint64_t tau_host[16];
  ST_TRY(read_constants(ctx, d_tau, nullptr, tau_host, nullptr));
  if (pol.use_gt) ST_TRY(b_table(ctx, pol.wb_b_req));
  return tau_table(ctx, pol.use_tables, d_tau, tau_host);
}
// per item: the ciphertext kernel, then GT_i = A^(r_i) B^(-beta_i r_i) with A = e(C, g2), B = e(g1, g2) (pairing.hip.h) or the pairing e(r_i (C - beta_i g1), g2), and the KDF
static keaki_status encap_items(keaki_hip_ctx* ctx, const EncapArgs& a, const EncapPolicy& pol, const uint64_t* tau_host, const AuxBuild& aux) {
  KemState& k = ctx->kem;
  void* gt = a.d_gt_out ? a.d_gt_out : ctx->tmp_b.p;
  const bool big = k.fb_tau.holds(tau_host);      // on the big-table path only, the ciphertext kernel shares its SIMDs with a table build on aux
  const KeyedTable<16>& tau = big ? k.fb_tau : k.fbs_tau;
  ST_TRY(encap_g2_fixed_run(ctx, tau.buf.p, tau.wb, (big ? k.fb_g2_gen : k.fbs_g2_gen).p, tau.wb, a.d_points, a.d_r, a.n, a.d_ct_out, big && aux.a_on_aux));
  if (pol.use_gt) {
    ST_TRY(wait_aux(ctx));
    // b_factor_done: the factor of the constant base ran while the commitment's table was on its way; the commitment's factor behind it
    if (aux.b_factor_done) ST_TRY(gt_encap_exp_run(ctx, k.gt_a.buf.p, k.gt_a.wb, nullptr, 0, a.d_values, a.d_r, a.n, gt, ctx->tmp_a.p, nullptr));
    else ST_TRY(gt_encap_exp_run(ctx, k.gt_a.buf.p, k.gt_a.wb, k.gt_tab_b.p, k.gt_b_wb, a.d_values, a.d_r, a.n, gt));
  } else {
    if (pol.use_tables) {
      ST_TRY(g1_fb_table_run(ctx, a.d_com, k.fb_com.p, FB_WB_BATCH));
      ST_TRY(encap_g1_fixed_run(ctx, k.fb_com.p, FB_WB_BATCH, k.fb_g1_gen.p, FB_WB_LONG, a.d_values, a.d_r, a.n, ctx->tmp_a.p));
    } else {
      ST_TRY(encap_g1_run(ctx, a.d_com, a.d_values, a.d_r, a.n, ctx->tmp_a.p));
    }
    ST_TRY(pairing_run(ctx, ctx->tmp_a.p, ctx->tmp_c.p, 0, a.n, gt, k.g2gen_lines.p));
  }
  if (a.d_key_out && a.msg_len) ST_TRY(blake3_gt_run(ctx, gt, a.n, a.d_key_out, a.msg_len, a.xor_into));
  return KEAKI_OK;
}
static keaki_status encap_impl(keaki_hip_ctx* ctx, const EncapArgs& a) {
  KemState& k = ctx->kem;
  // a chunk of a larger batch takes the decisions of the whole batch (table widths, the GT path) and counts as ONE call with its commitment
  const size_t n_policy = a.host ? a.host->n_batch : a.n;
  const bool first_of_batch = !a.host || a.host->first;
  ST_TRY(reserve(ctx, ctx->tmp_a, a.n * G1_AFF_BYTES));
  if (!a.d_gt_out) ST_TRY(reserve(ctx, ctx->tmp_b, a.n * 384));
  ST_TRY(generator_tables(ctx, n_policy >= FB_TABLES_MIN));
  uint64_t tau_dev[16], com_dev[8];
  const uint64_t *tau_host = a.host ? a.host->tau : tau_dev, *com_host = a.host ? a.host->com : com_dev;
  if (!a.host) ST_TRY(read_constants(ctx, a.d_tau, a.d_com, tau_dev, com_dev));
  note_commitment(k, com_host, first_of_batch);
  const EncapPolicy pol = encap_policy(n_policy, ctx->tune.gt_wb_b, ctx->tune.encap_gt, k.seen_com_runs, k.gt_b_ready && k.gt_a.holds(com_host), false);
  AuxBuild aux;
  if (pol.use_gt) {
    ST_TRY(b_table(ctx, pol.wb_b_req));
    ST_TRY(a_table(ctx, a, com_host, first_of_batch, &aux));
  }
  ST_TRY(tau_table(ctx, pol.use_tables, a.d_tau, tau_host));
  return encap_items(ctx, a, pol, tau_host, aux);
}
keaki_status keaki_hip_encap_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_tau_g2_aff, const void* d_points,
                                       const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff, void* d_gt_out, void* d_key_out,
                                       size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encap");
  if (n == 0) return KEAKI_OK;
  if (!d_com_aff || !d_tau_g2_aff || !d_points || !d_values || !d_r || !d_ct_out_aff || (!d_gt_out && !d_key_out) || msg_len > 65536)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_batch: bad argument");
  return encap_impl(ctx, {d_com_aff, d_tau_g2_aff, d_points, d_values, d_r, d_ct_out_aff, d_gt_out, d_key_out, n, msg_len});
}
// Setup-time: everything of encap_batch that depends on the setup only, for batches of `batch_hint` items (the KEM analogue of
// keaki_hip_srs_g1_precompute): fixed-base window tables of g1, g2 and [tau]_2, the line sequence of g2, and -- for hints >= 65,536 (or the
// threshold of option "encap_gt") -- the GT table of e(g1, g2) (2.6 GB; the 16-bit one when that does not fit). ~60 ms that the first
// large encap_batch of a context would otherwise pay. Results never depend on it.
keaki_status keaki_hip_encap_prepare(keaki_hip_ctx* ctx, const uint64_t* tau_g2_aff, size_t batch_hint) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encap_prepare");
  if (!tau_g2_aff) return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_prepare: null pointer");
  if (batch_hint == 0) return KEAKI_OK;
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_e, tau_g2_aff, 128));
  ST_TRY(kem_setup(ctx, ctx->io_e.p, batch_hint));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  feed.settled();
  return KEAKI_OK;
}
keaki_status keaki_hip_decap_batch_dev(keaki_hip_ctx* ctx, const void* d_proofs_aff, const void* d_cts_aff, size_t n, void* d_gt_out,
                                       void* d_key_out, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.decap");
  if (n == 0) return KEAKI_OK;
  if (!d_proofs_aff || !d_cts_aff || (!d_gt_out && !d_key_out) || msg_len > 65536) return fail(ctx, KEAKI_ERR_BAD_ARG, "decap_batch: bad argument");
  void* gt = d_gt_out;
  if (!gt) { ST_TRY(reserve(ctx, ctx->tmp_b, n * 384)); gt = ctx->tmp_b.p; }
  ST_TRY(pairing_run(ctx, d_proofs_aff, d_cts_aff, 1, n, gt));
  if (d_key_out && msg_len) ST_TRY(blake3_gt_run(ctx, gt, n, d_key_out, msg_len));
  return KEAKI_OK;
}
keaki_status keaki_hip_encap_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* points,
                                   const uint64_t* values, const uint64_t* r, size_t n, uint64_t* ct_out_aff, uint8_t* gt_out, uint8_t* key_out,
                                   size_t msg_len) {
  CTX_GUARD(ctx);                 // one lock from staging to the last download
  TRACE_SCOPE("keaki.encap");
  if (n == 0) return KEAKI_OK;
  if (!com_aff || !tau_g2_aff || !points || !values || !r || !ct_out_aff || (!gt_out && !key_out) || msg_len > 65536)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_batch: bad argument");
  const bool want_key = key_out && msg_len;
  return pipelined_regions(ctx, n, pipe_chunk_items(ctx, n), {{com_aff, nullptr, G1_AFF_BYTES}, {tau_g2_aff, nullptr, G2_AFF_BYTES}},
    {{points, nullptr, 32}, {values, nullptr, 32}, {r, nullptr, 32}, {nullptr, ct_out_aff, G2_AFF_BYTES}, {nullptr, gt_out, 384},
     {nullptr, want_key ? key_out : nullptr, msg_len}},
    [&](size_t lo, size_t m, char* const* hd, char* const* d) {
      const EncapHost eh = {com_aff, tau_g2_aff, n, lo == 0};
      return encap_impl(ctx, {hd[0], hd[1], d[0], d[1], d[2], d[3], d[4], want_key ? d[5] : nullptr, m, msg_len, false, &eh});
    });
}
keaki_status keaki_hip_decap_batch(keaki_hip_ctx* ctx, const uint64_t* proofs_aff, const uint64_t* cts_aff, size_t n, uint8_t* gt_out,
                                   uint8_t* key_out, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.decap");
  if (n == 0) return KEAKI_OK;
  if (!proofs_aff || !cts_aff || (!gt_out && !key_out) || msg_len > 65536) return fail(ctx, KEAKI_ERR_BAD_ARG, "decap_batch: bad argument");
  const bool want_key = key_out && msg_len;
  return pipelined_regions(ctx, n, pipe_chunk_items(ctx, n, pairing_launch_items()), {},
    {{proofs_aff, nullptr, G1_AFF_BYTES}, {cts_aff, nullptr, G2_AFF_BYTES}, {nullptr, gt_out, 384}, {nullptr, want_key ? key_out : nullptr, msg_len}},
    [&](size_t, size_t m, char* const*, char* const* d) -> keaki_status {
      ST_TRY(pairing_run(ctx, d[0], d[1], 1, m, d[2]));
      if (want_key) ST_TRY(blake3_gt_run(ctx, d[2], m, d[3], msg_len));
      return KEAKI_OK;
    });
}

// ---- enc::encrypt / enc::decrypt over a batch (src/enc.rs:19-55 inside the loops of src/vec.rs:63-66, :75-78): KEM + the XOR DEM on the device ----
// d_body_inout: n x msg_len bytes, the messages on entry and the ciphertext bodies on exit (decrypt: the other way round). The key is
// XORed in by the KDF kernel itself; neither GT bytes nor keys exist outside the device.
keaki_status keaki_hip_encrypt_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_tau_g2_aff, const void* d_points,
                                         const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff, void* d_body_inout, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encrypt");
  if (n == 0) return KEAKI_OK;
  if (!d_com_aff || !d_tau_g2_aff || !d_points || !d_values || !d_r || !d_ct_out_aff || !d_body_inout || msg_len == 0 || msg_len > 65536)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encrypt_batch: bad argument");
  return encap_impl(ctx, {d_com_aff, d_tau_g2_aff, d_points, d_values, d_r, d_ct_out_aff, nullptr, d_body_inout, n, msg_len, true});
}
keaki_status keaki_hip_decrypt_batch_dev(keaki_hip_ctx* ctx, const void* d_proofs_aff, const void* d_cts_aff, size_t n, void* d_body_inout, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.decrypt");
  if (n == 0) return KEAKI_OK;
  if (!d_proofs_aff || !d_cts_aff || !d_body_inout || msg_len == 0 || msg_len > 65536) return fail(ctx, KEAKI_ERR_BAD_ARG, "decrypt_batch: bad argument");
  ST_TRY(reserve(ctx, ctx->tmp_b, n * 384));
  ST_TRY(pairing_run(ctx, d_proofs_aff, d_cts_aff, 1, n, ctx->tmp_b.p));
  return blake3_gt_run(ctx, ctx->tmp_b.p, n, d_body_inout, msg_len, true);
}
keaki_status keaki_hip_encrypt_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* points,
                                     const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n, uint64_t* ct_out_aff, uint8_t* body_out,
                                     size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encrypt");
  if (n == 0) return KEAKI_OK;
  if (!com_aff || !tau_g2_aff || !points || !values || !r || !msgs || !ct_out_aff || !body_out || msg_len == 0 || msg_len > 65536)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encrypt_batch: bad argument");
  return pipelined_regions(ctx, n, pipe_chunk_items(ctx, n), {{com_aff, nullptr, G1_AFF_BYTES}, {tau_g2_aff, nullptr, G2_AFF_BYTES}},
    {{points, nullptr, 32}, {values, nullptr, 32}, {r, nullptr, 32}, {nullptr, ct_out_aff, G2_AFF_BYTES}, {msgs, body_out, msg_len}},
    [&](size_t lo, size_t m, char* const* hd, char* const* d) {
      const EncapHost eh = {com_aff, tau_g2_aff, n, lo == 0};
      return encap_impl(ctx, {hd[0], hd[1], d[0], d[1], d[2], d[3], nullptr, d[4], m, msg_len, true, &eh});
    });
}
keaki_status keaki_hip_decrypt_batch(keaki_hip_ctx* ctx, const uint64_t* proofs_aff, const uint64_t* cts_aff, const uint8_t* bodies, size_t n,
                                     uint8_t* msgs_out, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.decrypt");
  if (n == 0) return KEAKI_OK;
  if (!proofs_aff || !cts_aff || !bodies || !msgs_out || msg_len == 0 || msg_len > 65536) return fail(ctx, KEAKI_ERR_BAD_ARG, "decrypt_batch: bad argument");
  const size_t ch = pipe_chunk_items(ctx, n, pairing_launch_items());
  ST_TRY(reserve(ctx, ctx->tmp_b, ch * 384));            // the GT values stay on the device
  return pipelined_regions(ctx, n, ch, {}, {{proofs_aff, nullptr, G1_AFF_BYTES}, {cts_aff, nullptr, G2_AFF_BYTES}, {bodies, msgs_out, msg_len}},
    [&](size_t, size_t m, char* const*, char* const* d) -> keaki_status {
      ST_TRY(pairing_run(ctx, d[0], d[1], 1, m, ctx->tmp_b.p));
      return blake3_gt_run(ctx, ctx->tmp_b.p, m, d[2], msg_len, true);
    });
}

// ---- encap_multi / encrypt_multi: the sender's side of a many-party flow, a commitment per GROUP of items (src/vec.rs:52-69 once per receiver) ----
// A group of at least "encap_multi_single_min" items runs the single-commitment path above on its item range (encap_impl: GT tables, 1.7 ms
// and 31.5 MB for a commitment seen for the first time). Every other item runs the FUSED route, in maximal runs of consecutive small groups
// (encap_multi_plan.h): the ciphertext kernel as it is, one G1 kernel that finds each item's commitment from the offsets (kem_multi.hip), a
// pairing per item against g2's tabulated lines and the KDF. The fused route builds no table per commitment and leaves seen_com, gt_a and
// fb_com of KemState alone; table widths follow the size of the WHOLE call, as the chunks of a host batch follow their batch.
// d_coms / d_offsets: the commitments and offsets of the run's groups (n_groups, n_groups + 1 words); `first`: global index of the first item
struct EncapMultiRun { const void *d_coms, *d_offsets; size_t n_groups; uint64_t first; };
static keaki_status encap_multi_fused(keaki_hip_ctx* ctx, const EncapMultiRun& run, const EncapArgs& a, size_t n_policy, const uint64_t* tau_host) {
  KemState& k = ctx->kem;
  const bool use_tables = n_policy >= FB_TABLES_MIN;
  ST_TRY(reserve(ctx, ctx->tmp_a, a.n * G1_AFF_BYTES));
  if (!a.d_gt_out) ST_TRY(reserve(ctx, ctx->tmp_b, a.n * 384));
  ST_TRY(generator_tables(ctx, use_tables));
  ST_TRY(tau_table(ctx, use_tables, a.d_tau, tau_host));
  if (!k.fb_ready) ST_TRY(small_g1_table(ctx));
  void* gt = a.d_gt_out ? a.d_gt_out : ctx->tmp_b.p;
  const bool big = k.fb_tau.holds(tau_host);
  const KeyedTable<16>& tau = big ? k.fb_tau : k.fbs_tau;
  ST_TRY(encap_g2_fixed_run(ctx, tau.buf.p, tau.wb, (big ? k.fb_g2_gen : k.fbs_g2_gen).p, tau.wb, a.d_points, a.d_r, a.n, a.d_ct_out));
  ST_TRY(encap_multi_g1_run(ctx, run.d_coms, run.d_offsets, run.n_groups, run.first, (k.fb_ready ? k.fb_g1_gen : k.fbs_g1_gen).p,
                            k.fb_ready ? FB_WB_LONG : FB_WB_SMALL, a.d_values, a.d_r, a.n, ctx->tmp_a.p));
  ST_TRY(pairing_run(ctx, ctx->tmp_a.p, ctx->tmp_c.p, 0, a.n, gt, k.g2gen_lines.p));
  if (a.d_key_out && a.msg_len) ST_TRY(blake3_gt_run(ctx, gt, a.n, a.d_key_out, a.msg_len, a.xor_into));
  return KEAKI_OK;
}
// items [lo, lo + n) of the caller's per-item arrays (device)
static EncapArgs encap_multi_slice(const EncapArgs& a, size_t lo, size_t n) {
  EncapArgs s = a;
  s.d_points = (const char*)a.d_points + lo * 32; s.d_values = (const char*)a.d_values + lo * 32; s.d_r = (const char*)a.d_r + lo * 32;
  s.d_ct_out = (char*)a.d_ct_out + lo * G2_AFF_BYTES;
  if (a.d_gt_out) s.d_gt_out = (char*)a.d_gt_out + lo * 384;
  if (a.d_key_out) s.d_key_out = (char*)a.d_key_out + lo * a.msg_len;
  s.n = n;
  return s;
}
// `a` holds the arrays of ALL items (d_com: the m commitments); offsets: the caller's HOST array, validated
static keaki_status encap_multi_dev(keaki_hip_ctx* ctx, const EncapArgs& a, const uint64_t* offsets, size_t m) {
  const std::vector<EncapMultiPiece> pieces = encap_multi_plan(offsets, m, ctx->tune.encap_multi_single_min);
  // the offsets go up in front of the one read-back, whose synchronisation also ends the read of the caller's array
  ST_TRY(reserve(ctx, ctx->em_offsets, (m + 1) * 8));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->em_offsets.p, offsets, (m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  uint64_t tau_host[16];
  ST_TRY(read_constants(ctx, a.d_tau, nullptr, tau_host, nullptr));
  for (const EncapMultiPiece& p : pieces) {
    if (p.i_hi == p.i_lo) continue;
    EncapArgs s = encap_multi_slice(a, p.i_lo, p.i_hi - p.i_lo);
    if (p.single) {
      s.d_com = (const char*)a.d_com + p.g_lo * G1_AFF_BYTES;
      ST_TRY(encap_impl(ctx, s));                          // reads this group's commitment back: it keys the GT table
    } else {
      const EncapMultiRun run = {(const char*)a.d_com + p.g_lo * G1_AFF_BYTES, (const char*)ctx->em_offsets.p + p.g_lo * 8, p.g_hi - p.g_lo, p.i_lo};
      ST_TRY(encap_multi_fused(ctx, run, s, a.n, tau_host));
    }
  }
  return KEAKI_OK;
}
keaki_status keaki_hip_encap_multi_dev(keaki_hip_ctx* ctx, const void* d_coms_aff, const uint64_t* offsets, size_t m, const void* d_tau_g2_aff,
                                       const void* d_points, const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff, void* d_gt_out,
                                       void* d_key_out, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encap_multi");
  if (n == 0) return KEAKI_OK;
  if (!d_coms_aff || !d_tau_g2_aff || !d_points || !d_values || !d_r || !d_ct_out_aff || (!d_gt_out && !d_key_out) || msg_len > 65536 ||
      !encap_multi_offsets_ok(offsets, m, n))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_multi: bad argument");
  return encap_multi_dev(ctx, {d_coms_aff, d_tau_g2_aff, d_points, d_values, d_r, d_ct_out_aff, d_gt_out, d_key_out, n, msg_len}, offsets, m);
}
keaki_status keaki_hip_encrypt_multi_dev(keaki_hip_ctx* ctx, const void* d_coms_aff, const uint64_t* offsets, size_t m, const void* d_tau_g2_aff,
                                         const void* d_points, const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff,
                                         void* d_body_inout, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encrypt_multi");
  if (n == 0) return KEAKI_OK;
  if (!d_coms_aff || !d_tau_g2_aff || !d_points || !d_values || !d_r || !d_ct_out_aff || !d_body_inout || msg_len == 0 || msg_len > 65536 ||
      !encap_multi_offsets_ok(offsets, m, n))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encrypt_multi: bad argument");
  return encap_multi_dev(ctx, {d_coms_aff, d_tau_g2_aff, d_points, d_values, d_r, d_ct_out_aff, nullptr, d_body_inout, n, msg_len, true}, offsets, m);
}
// Host forms. A fused run is ONE pipelined batch with the run's commitments, its offsets and [tau]_2 as head constants (a chunk may begin
// anywhere inside a group: the kernel takes the global index of the chunk's first item); a large group is the single-commitment host call
// on its sub-range of the caller's arrays. Each piece fences its own copies, so a failing call returns with nothing in flight.
// Chunks of a fused run: 2^15 items (4.6 ms of pairings at 7.1 M/s against 3 MB up and up to 17 MB down), from two chunks on. Not measured against 2^16 / 2^17.
constexpr size_t ENCAP_MULTI_CHUNK = 32768;
// msgs: null for encap (gt / key out), else the messages of encrypt (bodies to key_or_body_out)
static keaki_status encap_multi_host(keaki_hip_ctx* ctx, const uint64_t* coms, const uint64_t* offsets, size_t m, const uint64_t* tau, const uint64_t* points,
                                     const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n, uint64_t* ct_out, uint8_t* gt_out,
                                     uint8_t* key_or_body_out, size_t msg_len) {
  const bool want_key = key_or_body_out && msg_len;
  for (const EncapMultiPiece& p : encap_multi_plan(offsets, m, ctx->tune.encap_multi_single_min)) {
    const size_t lo = p.i_lo, cnt = p.i_hi - p.i_lo;
    if (!cnt) continue;
    const uint64_t *pts = points + lo * 4, *vals = values + lo * 4, *rs = r + lo * 4;
    uint64_t* ct = ct_out + lo * 16;
    uint8_t* gt = gt_out ? gt_out + lo * 384 : nullptr;
    uint8_t* kb = key_or_body_out ? key_or_body_out + lo * msg_len : nullptr;
    const uint8_t* ms = msgs ? msgs + lo * msg_len : nullptr;
    if (p.single) {
      ST_TRY(msgs ? keaki_hip_encrypt_batch(ctx, coms + p.g_lo * 8, tau, pts, vals, rs, ms, cnt, ct, kb, msg_len)
                  : keaki_hip_encap_batch(ctx, coms + p.g_lo * 8, tau, pts, vals, rs, cnt, ct, gt, kb, msg_len));
      continue;
    }
    const size_t ng = p.g_hi - p.g_lo;
    ST_TRY(pipelined_regions(ctx, cnt, pipe_chunk_items(ctx, cnt, ENCAP_MULTI_CHUNK),
      {{coms + p.g_lo * 8, nullptr, ng * G1_AFF_BYTES}, {tau, nullptr, G2_AFF_BYTES}, {offsets + p.g_lo, nullptr, (ng + 1) * 8}},
      {{pts, nullptr, 32}, {vals, nullptr, 32}, {rs, nullptr, 32}, {nullptr, ct, G2_AFF_BYTES}, {nullptr, gt, msgs ? 0 : (size_t)384},
       {ms, want_key ? kb : nullptr, msg_len}},
      [&](size_t clo, size_t cm, char* const* hd, char* const* d) {
        const EncapMultiRun run = {hd[0], hd[2], ng, lo + clo};
        // encrypt keeps its GT values in the context's workspace (d_gt_out null), as encrypt_batch does
        return encap_multi_fused(ctx, run, {nullptr, hd[1], d[0], d[1], d[2], d[3], msgs ? nullptr : d[4], want_key ? d[5] : nullptr, cm, msg_len, msgs != nullptr},
                                 n, tau);
      }));
  }
  return KEAKI_OK;
}
keaki_status keaki_hip_encap_multi(keaki_hip_ctx* ctx, const uint64_t* coms_aff, const uint64_t* offsets, size_t m, const uint64_t* tau_g2_aff,
                                   const uint64_t* points, const uint64_t* values, const uint64_t* r, size_t n, uint64_t* ct_out_aff, uint8_t* gt_out,
                                   uint8_t* key_out, size_t msg_len) {
  CTX_GUARD(ctx);                 // one lock over every piece of the call
  TRACE_SCOPE("keaki.encap_multi");
  if (n == 0) return KEAKI_OK;
  if (!coms_aff || !tau_g2_aff || !points || !values || !r || !ct_out_aff || (!gt_out && !key_out) || msg_len > 65536 ||
      !encap_multi_offsets_ok(offsets, m, n))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encap_multi: bad argument");
  return encap_multi_host(ctx, coms_aff, offsets, m, tau_g2_aff, points, values, r, nullptr, n, ct_out_aff, gt_out, key_out, msg_len);
}
keaki_status keaki_hip_encrypt_multi(keaki_hip_ctx* ctx, const uint64_t* coms_aff, const uint64_t* offsets, size_t m, const uint64_t* tau_g2_aff,
                                     const uint64_t* points, const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n,
                                     uint64_t* ct_out_aff, uint8_t* body_out, size_t msg_len) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.encrypt_multi");
  if (n == 0) return KEAKI_OK;
  if (!coms_aff || !tau_g2_aff || !points || !values || !r || !msgs || !ct_out_aff || !body_out || msg_len == 0 || msg_len > 65536 ||
      !encap_multi_offsets_ok(offsets, m, n))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "encrypt_multi: bad argument");
  return encap_multi_host(ctx, coms_aff, offsets, m, tau_g2_aff, points, values, r, msgs, n, ct_out_aff, nullptr, body_out, msg_len);
}

// ---- FK23 batch openings: replaces kzg::open_fk (src/kzg.rs:157-203) ----------------------------------------------------------
keaki_status keaki_hip_open_fk(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* hat_a, const uint64_t* tw_2d,
                               const uint64_t* tw_2d_inv, const uint64_t* tw_d, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fk_enter(ctx, srs, log2d, hat_a && tw_2d && tw_2d_inv && proofs_out_aff, "open_fk", hl));
  const size_t d = (size_t)1 << log2d;
  // one staging buffer: hat_a (2d Fr) | tw_2d (d) | tw_2d_inv (d) | tw_d (d/2) | work (2d Jacobian) | proofs (d affine)
  const size_t o_ha = 0, o_t1 = o_ha + 2 * d * 32, o_t2 = o_t1 + d * 32, o_t3 = o_t2 + d * 32, o_w = o_t3 + (d / 2 + 1) * 32, o_p = o_w + open_fk_poly_g_bytes(log2d),
               total = o_p + d * 64;
  ST_TRY(reserve(ctx, ctx->io_d, total));
  char* b = (char*)ctx->io_d.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, b + o_ha, hat_a, 2 * d * 32));
  ST_TRY(feed.put(0, b + o_t1, tw_2d, d * 32));
  ST_TRY(feed.put(0, b + o_t2, tw_2d_inv, d * 32));
  (void)tw_d;                       // the size-d transforms take every second entry of the 2d tables
  ST_TRY(fk_cache_ensure(ctx, srs, log2d, b + o_t1));
  ST_TRY(open_fk_run(ctx, srs->fk.p, log2d, b + o_ha, b + o_t1, b + o_t2, b + o_w, b + o_p));
  prefault_out(ctx, proofs_out_aff, d * 64);
  return download(feed, proofs_out_aff, b + o_p, d * 64);
}

// FK23 from the coefficients: twiddles and hat_a are derived on the device (row f-4)
keaki_status keaki_hip_open_fk_poly(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* coeffs, const uint64_t* omega_2d,
                                    const uint64_t* omega_2d_inv, const uint64_t* inv_2d, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fk_enter(ctx, srs, log2d, coeffs && omega_2d && omega_2d_inv && inv_2d && proofs_out_aff, "open_fk_poly", hl));
  const size_t d = (size_t)1 << log2d;
  // one staging block: coefficients (d Fr) | FK23 scalar work | FK23 point work | proofs (d affine)
  const size_t o_p = 0, o_fr = o_p + d * 32, o_g = o_fr + open_fk_poly_fr_bytes(log2d), o_out = o_g + open_fk_poly_g_bytes(log2d), total = o_out + d * 64;
  ST_TRY(reserve(ctx, ctx->io_d, total));
  char* b = (char*)ctx->io_d.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, b + o_p, coeffs, d * 32));
  ST_TRY(open_fk_from_poly(ctx, srs, log2d, b + o_p, omega_2d, omega_2d_inv, inv_2d, b + o_fr, b + o_g, b + o_out));
  prefault_out(ctx, proofs_out_aff, d * 64);
  return download(feed, proofs_out_aff, b + o_out, d * 64);
}
// hat_s = DFT_2d(reversed SRS) for later open_fk calls with this d: setup-time work (the FK23 analogue of keaki_hip_srs_g1_precompute)
keaki_status keaki_hip_srs_g1_precompute_fk(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_2d) {
  CTX_GUARD(ctx);
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fk_enter(ctx, srs, log2d, omega_2d != nullptr, "srs_g1_precompute_fk", hl));
  const uint32_t d = 1u << log2d;
  ST_TRY(reserve(ctx, ctx->io_d, (size_t)d * 32));
  if (!srs->fk.holds((int)log2d)) {
    fr_powers_run(ctx, omega_2d, d, ctx->io_d.p);
    ST_TRY(fk_cache_ensure(ctx, srs, log2d, ctx->io_d.p));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // setup-time call: return when the table exists
  return KEAKI_OK;
}
// ---- FK23 coset openings: all d / l set proofs of the l-point cosets in one call (fk_coset.hip) ------------------------------------------------
namespace {
// the l coset transforms of (d, l) = (2^log2d, 2^log2l), r = d / l >= 2, into srs->fkc. d_tw: omega_2r^k, k < r, ready in stream order
keaki_status fkc_cache_ensure(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const void* d_tw) {
  return srs_cache_ensure(ctx, srs, srs->fkc, (int)log2d, (int)log2l, ((size_t)2 << log2d) * G1_JAC_BYTES,
                          [&](void* hat_s) { return fkc_hat_s_run(ctx, srs->d, log2d, log2l, d_tw, hat_s); });
}
// One call of the coset openings on device data. Exactly one of d_coeffs (d Fr) and d_hat_a (l rows of 2r Fr) is given; `host` stages it from the caller's
// array and downloads the r proofs to proofs_out, else d_out receives them in stream order. Every allocation that can be refused (workspaces, the
// handle's transforms) comes before the first copy and before any kernel that writes an output.
struct FkcCall {
  uint32_t log2d, log2l;
  const uint64_t *omega_2r, *omega_2r_inv, *inv_2r;      // inv_2r: null for the raw hat_a form
};
keaki_status fkc_call(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const FkcCall& k, const void* coeffs, const void* hat_a, bool host, void* out) {
  const uint32_t log2r = k.log2d - k.log2l, l = 1u << k.log2l;
  const size_t d = (size_t)1 << k.log2d, r = (size_t)1 << log2r;
  if (r == 1) {                                           // deg p < d = l: the one quotient is zero
    if (host) { memset(out, 0, G1_AFF_BYTES); return KEAKI_OK; }
    HIP_TRY(ctx, hipMemsetAsync(out, 0, G1_AFF_BYTES, ctx->stream));
    return KEAKI_OK;
  }
  const FkcPlan plan = fkc_plan(2 * r, l, (uint32_t)ctx->tune.fk_coset_group, (uint64_t)ctx->tune.fk_coset_min_lanes);
  // one block: scalar work | point work | host forms: coefficients (d Fr) and proofs (r affine)
  const size_t o_fr = 0, o_g = o_fr + fkc_fr_bytes(k.log2d, k.log2l), o_in = o_g + fkc_g_bytes(k.log2d, k.log2l, plan), o_out = o_in + (host && coeffs ? d * 32 : 0),
               total = o_out + (host ? r * G1_AFF_BYTES : 0);
  ST_TRY(reserve(ctx, ctx->fc_work, total));
  uint32_t per_launch = 0;
  ST_TRY(fkc_reserve_tab(ctx, (size_t)plan.S * 2 * r, plan.G, &per_launch));
  char* b = (char*)ctx->fc_work.p;
  const FkcScalars s = fkc_layout(k.log2d, k.log2l, b + o_fr);
  ST_TRY(fkc_tables_run(ctx, log2r, k.omega_2r, k.omega_2r_inv, s));
  ST_TRY(fkc_cache_ensure(ctx, srs, k.log2d, k.log2l, s.tw));
  CopyFeed feed(ctx);
  const void* d_p = coeffs;
  if (host && coeffs) { ST_TRY(feed.put(0, b + o_in, coeffs, d * 32)); d_p = b + o_in; }
  if (hat_a) {
    if (host) ST_TRY(feed.put(0, s.hat_a, hat_a, 2 * d * 32));
    else HIP_TRY(ctx, hipMemcpyAsync(s.hat_a, hat_a, 2 * d * 32, hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    ST_TRY(fkc_scalars_run(ctx, k.log2d, k.log2l, d_p, k.inv_2r, s));
  }
  ST_TRY(fkc_open_run(ctx, srs->fkc.p, k.log2d, k.log2l, s, plan, per_launch, b + o_g, host ? (void*)(b + o_out) : out));
  if (!host) return KEAKI_OK;
  prefault_out(ctx, out, r * G1_AFF_BYTES);
  return download(feed, out, b + o_out, r * G1_AFF_BYTES);
}
// how the coset entries start: fk_enter's checks, and l = 2^log2l <= min(d, KEAKI_SET_MAX)
keaki_status fkc_enter(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, bool args_ok, const char* what,
                       std::unique_lock<std::recursive_mutex>& hl) {
  const bool l_ok = log2l <= log2d && log2l < 32 && ((uint64_t)1 << log2l) <= (uint64_t)KEAKI_SET_MAX;
  return fk_enter(ctx, srs, log2d, args_ok && l_ok, what, hl);
}
}  // namespace
keaki_status keaki_hip_srs_g1_precompute_fk_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* omega_2r) {
  CTX_GUARD(ctx);
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fkc_enter(ctx, srs, log2d, log2l, omega_2r != nullptr, "srs_g1_precompute_fk_cosets", hl));
  if (log2d == log2l) return KEAKI_OK;                    // r = 1: the call needs no transform
  const uint32_t r = 1u << (log2d - log2l);
  ST_TRY(reserve(ctx, ctx->io_d, (size_t)r * 32));
  if (!srs->fkc.holds((int)log2d, (int)log2l)) {
    fr_powers_run(ctx, omega_2r, r, ctx->io_d.p);
    ST_TRY(fkc_cache_ensure(ctx, srs, log2d, log2l, ctx->io_d.p));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // setup-time call: return when the rows exist
  return KEAKI_OK;
}
keaki_status keaki_hip_open_fk_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* hat_a, const uint64_t* omega_2r,
                                      const uint64_t* omega_2r_inv, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk_cosets");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fkc_enter(ctx, srs, log2d, log2l, hat_a && omega_2r && omega_2r_inv && proofs_out_aff, "open_fk_cosets", hl));
  return fkc_call(ctx, srs, {log2d, log2l, omega_2r, omega_2r_inv, nullptr}, nullptr, hat_a, true, proofs_out_aff);
}
keaki_status keaki_hip_open_fk_cosets_poly(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* coeffs,
                                           const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const uint64_t* inv_2r, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk_cosets");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fkc_enter(ctx, srs, log2d, log2l, coeffs && omega_2r && omega_2r_inv && inv_2r && proofs_out_aff, "open_fk_cosets_poly", hl));
  return fkc_call(ctx, srs, {log2d, log2l, omega_2r, omega_2r_inv, inv_2r}, coeffs, nullptr, true, proofs_out_aff);
}
keaki_status keaki_hip_open_fk_cosets_poly_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const void* d_coeffs,
                                               const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const uint64_t* inv_2r, void* d_proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk_cosets");
  std::unique_lock<std::recursive_mutex> hl;
  const bool aligned = !(((uintptr_t)d_coeffs | (uintptr_t)d_proofs_out_aff) & 15);
  ST_TRY(fkc_enter(ctx, srs, log2d, log2l, d_coeffs && omega_2r && omega_2r_inv && inv_2r && d_proofs_out_aff && aligned, "open_fk_cosets_poly_dev", hl));
  return fkc_call(ctx, srs, {log2d, log2l, omega_2r, omega_2r_inv, inv_2r}, d_coeffs, nullptr, false, d_proofs_out_aff);
}
// In-place scalar-field DFT of n = 2^log2n elements with the order-n root `omega`, then an optional scaling (the 1/n of an inverse transform).
keaki_status keaki_hip_fr_fft(keaki_hip_ctx* ctx, uint64_t* data, uint32_t log2n, const uint64_t* omega, const uint64_t* scale_or_null) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.fr_fft");
  if (!data || !omega || log2n > 28) return fail(ctx, KEAKI_ERR_BAD_ARG, "fr_fft: bad argument");
  const size_t n = (size_t)1 << log2n;
  ST_TRY(reserve(ctx, ctx->io_d, n * 32 + (n / 2 + 1) * 32));
  char* b = (char*)ctx->io_d.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, b, data, n * 32));
  ST_TRY(fr_fft_run(ctx, b, log2n, omega, scale_or_null, b + n * 32));
  return download(feed, data, b, n * 32);
}

// ---- vec_commit in one call (src/vec.rs:22-49 behind the padding draw): iFFT -> FK23 openings -> commit, coefficients never leave the device ----
keaki_status keaki_hip_vec_commit(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const uint64_t* values, size_t n, const uint64_t* pad, uint32_t log2d,
                                  const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                                  const uint64_t* inv_2d, uint64_t* com_out_jac, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.vec_commit");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(fk_enter(ctx, srs, log2d, (!n || values) && omega_d_inv && inv_d && omega_2d && omega_2d_inv && inv_2d && com_out_jac && proofs_out_aff, "vec_commit", hl));
  const size_t d = (size_t)1 << log2d, m = n + (pad ? 1 : 0);
  if (m > d) return fail(ctx, KEAKI_ERR_BAD_ARG, "vec_commit: %zu evaluations do not fit the domain of %zu", m, d);
  // one staging block: coefficients (d Fr) | twiddles of the iFFT (d/2 + 1) | FK23 scalar work | FK23 point work (2d Jacobian) | proofs (d affine) | commitment
  const size_t o_c = 0, o_tw = o_c + d * 32, o_fr = o_tw + (d / 2 + 1) * 32, o_g = o_fr + open_fk_poly_fr_bytes(log2d), o_out = o_g + open_fk_poly_g_bytes(log2d),
               o_com = o_out + d * 64, total = o_com + 96;
  ST_TRY(reserve(ctx, ctx->io_d, total));
  char* b = (char*)ctx->io_d.p;
  hipStream_t st = ctx->stream;
  if (m < d) HIP_TRY(ctx, hipMemsetAsync(b + o_c + m * 32, 0, (d - m) * 32, st));          // evaluations beyond the padded vector are zero (ark-poly's ifft resizes)
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, b + o_c, values, n * 32));
  if (pad) ST_TRY(feed.put(0, b + o_c + n * 32, pad, 32));
  ST_TRY(fr_fft_run(ctx, b + o_c, log2d, omega_d_inv, inv_d, b + o_tw));                  // domain.ifft (src/vec.rs:37)
  ST_TRY(open_fk_from_poly(ctx, srs, log2d, b + o_c, omega_2d, omega_2d_inv, inv_2d, b + o_fr, b + o_g, b + o_out));   // :40
  const auto tb = srs_tables(srs);
  ST_TRY(msm_g1_run(ctx, srs->d, srs->n, b + o_c, d, b + o_com, tb.first, tb.second));     // :46 (trailing zero coefficients contribute nothing)
  prefault_out(ctx, proofs_out_aff, d * 64);
  HIP_TRY(ctx, hipMemcpyAsync(com_out_jac, b + o_com, 96, hipMemcpyDeviceToHost, st));
  ST_TRY(download(feed, proofs_out_aff, b + o_out, d * 64));
  resolve_timing(ctx);
  return KEAKI_OK;
}

// ---- vec_update: k evaluations of a committed vector change, the commitment and all d proofs follow (vec_update.hip) -------------------------
namespace {
// the update tables of d = 2^log2d into srs->upd
keaki_status upd_cache_ensure(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d_inv, const uint64_t* inv_d) {
  return srs_cache_ensure(ctx, srs, srs->upd, (int)log2d, -1, upd_table_bytes(log2d),
                          [&](void* tab) { return upd_tables_run(ctx, srs->d, log2d, omega_d_inv, inv_d, tab); });
}
constexpr const char* SRS_SHORT_UPD = "vec_update: a domain of %zu but the SRS holds %zu points";
// how the three entries start: fk_enter's checks with vec_update's message, and k < 2^31
keaki_status upd_enter(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, bool args_ok, size_t k, const char* what, std::unique_lock<std::recursive_mutex>& hl) {
  return fk_enter(ctx, srs, log2d, args_ok && k < ((size_t)1 << 31), what, hl, SRS_SHORT_UPD);
}
}  // namespace
keaki_status keaki_hip_srs_g1_precompute_update(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                                const uint64_t* inv_d) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.vec_update_tables");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(upd_enter(ctx, srs, log2d, omega_d && omega_d_inv && inv_d, 0, "srs_g1_precompute_update", hl));
  ST_TRY(upd_cache_ensure(ctx, srs, log2d, omega_d_inv, inv_d));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // setup-time call: return when the tables exist
  return KEAKI_OK;
}
keaki_status keaki_hip_vec_update_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                      const uint64_t* inv_d, const void* d_idx, const void* d_deltas, size_t k, void* d_com_inout_jac, void* d_proofs_inout_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.vec_update");
  std::unique_lock<std::recursive_mutex> hl;
  const bool aligned = !(((uintptr_t)d_idx & 3) | (((uintptr_t)d_deltas | (uintptr_t)d_com_inout_jac | (uintptr_t)d_proofs_inout_aff) & 15));
  ST_TRY(upd_enter(ctx, srs, log2d, omega_d && omega_d_inv && inv_d && (!k || (d_idx && d_deltas)) && aligned, k, "vec_update_dev", hl));
  if (k == 0 || (!d_com_inout_jac && !d_proofs_inout_aff)) return KEAKI_OK;
  ST_TRY(upd_cache_ensure(ctx, srs, log2d, omega_d_inv, inv_d));
  return upd_apply_run(ctx, srs->upd.p, log2d, inv_d, d_idx, d_deltas, k, d_com_inout_jac, d_proofs_inout_aff);
}
keaki_status keaki_hip_vec_update(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                  const uint64_t* inv_d, const uint32_t* idx, const uint64_t* deltas, size_t k, uint64_t* com_inout_jac, uint64_t* proofs_inout_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.vec_update");
  std::unique_lock<std::recursive_mutex> hl;
  ST_TRY(upd_enter(ctx, srs, log2d, omega_d && omega_d_inv && inv_d && (!k || (idx && deltas)), k, "vec_update", hl));
  const size_t d = (size_t)1 << log2d;
  for (size_t t = 0; t < k; t++)
    if (idx[t] >= d) return fail(ctx, KEAKI_ERR_BAD_ARG, "vec_update: index %u (entry %zu) is outside the domain of %zu", idx[t], t, d);
  if (k == 0 || (!com_inout_jac && !proofs_inout_aff)) return KEAKI_OK;
  // one staging block: deltas (k Fr) | commitment | proofs (d affine) | indices (k u32)
  const size_t o_dl = 0, o_com = o_dl + k * 32, o_pr = o_com + 96, o_ix = o_pr + (proofs_inout_aff ? d * 64 : 0), total = o_ix + k * 4;
  ST_TRY(reserve(ctx, ctx->vu_io, total));
  ST_TRY(upd_cache_ensure(ctx, srs, log2d, omega_d_inv, inv_d));       // before the first copy: a refused table leaves nothing behind
  char* b = (char*)ctx->vu_io.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, b + o_dl, deltas, k * 32));
  ST_TRY(feed.put(0, b + o_ix, idx, k * 4));
  if (com_inout_jac) ST_TRY(feed.put(0, b + o_com, com_inout_jac, 96));
  if (proofs_inout_aff) ST_TRY(feed.put(0, b + o_pr, proofs_inout_aff, d * 64));
  ST_TRY(upd_apply_run(ctx, srs->upd.p, log2d, inv_d, b + o_ix, b + o_dl, k, com_inout_jac ? b + o_com : nullptr, proofs_inout_aff ? b + o_pr : nullptr));
  // both outputs in one download when both are asked for (they are neighbours in the block)
  if (com_inout_jac && !proofs_inout_aff) return download(feed, com_inout_jac, b + o_com, 96);
  if (com_inout_jac) HIP_TRY(ctx, hipMemcpyAsync(com_inout_jac, b + o_com, 96, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, proofs_inout_aff, b + o_pr, d * 64);
}

// ---- FK23 sharded over `world` = 2^k ranks: one handle per rank, the caller runs the exchanges between the steps -----------------
struct keaki_hip_fk_shard {
  FkShard plan;
  const keaki_hip_srs_g1* srs = nullptr;      // must outlive the handle
  uint32_t world = 0;
  int setup_next = 0, open_next = 0;          // the step each sequence expects next (a skipped exchange cannot be detected, a skipped step can)
};
namespace {
size_t fk_shard_buffer_bytes(const keaki_hip_fk_shard* fk) {
  const size_t d = (size_t)1 << fk->plan.log2d;
  return std::max(2 * d / fk->world * 96, d * 64);
}
void fk_shard_release(keaki_hip_fk_shard* fk) {
  for (void** p : {&fk->plan.tw, &fk->plan.twi, &fk->plan.hat_a, &fk->plan.coeffs, &fk->plan.hat_s, &fk->plan.work, &fk->plan.e})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
}
}  // namespace
keaki_status keaki_hip_fk_shard_create(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t rank, uint32_t world,
                                       const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d, keaki_hip_fk_shard** out) {
  CTX_GUARD(ctx);
  if (!srs || !omega_2d || !omega_2d_inv || !inv_2d || !out || log2d > 27) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_create: bad argument");
  *out = nullptr;
  if (world < 2 || (world & (world - 1)) || rank >= world) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_create: world = %u must be a power of two >= 2, rank %u below it", world, rank);
  const size_t d = (size_t)1 << log2d;
  if (d < (size_t)world * world)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_create: %zu openings are too few to shard over %u ranks (needs world^2); use keaki_hip_open_fk_poly", d, world);
  ST_TRY(srs_holds(ctx, srs, "fk_shard_create", d, SRS_SHORT_FK));
  auto* fk = new keaki_hip_fk_shard();
  fk->srs = srs;
  fk->world = world;
  fk->plan.log2d = log2d;
  fk->plan.rank = rank;
  while ((1u << fk->plan.rho) < world) fk->plan.rho++;
  memcpy(fk->plan.omega, omega_2d, 32); memcpy(fk->plan.omega_inv, omega_2d_inv, 32); memcpy(fk->plan.inv_2d, inv_2d, 32);
  const size_t m = 2 * d / world;
  keaki_status st = KEAKI_OK;
  const std::pair<void**, size_t> want[] = {{&fk->plan.tw, d * 32}, {&fk->plan.twi, d * 32}, {&fk->plan.hat_a, 2 * d * 32}, {&fk->plan.coeffs, d * 32},
                                            {&fk->plan.hat_s, m * 96}, {&fk->plan.work, m * 96}, {&fk->plan.e, m / 2 * 96}};
  for (auto& w : want)
    if (st == KEAKI_OK) st = dev_alloc(ctx, w.first, w.second);
  if (st != KEAKI_OK) { fk_shard_release(fk); delete fk; return st; }
  *out = fk;
  return KEAKI_OK;
}
void keaki_hip_fk_shard_free(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk) {
  if (!fk) return;
  keaki_internal::DeviceScope dev_(ctx ? ctx->device : fk->srs ? fk->srs->device : -1);
  if (ctx) {
    std::lock_guard<std::recursive_mutex> lock_(ctx->mu);
    (void)hipStreamSynchronize(ctx->stream);
  } else if (fk->srs && fk->srs->device >= 0) {
    (void)hipDeviceSynchronize();
  }
  fk_shard_release(fk);             // hipFree needs no context: the device buffers go even when the caller's ctx is already gone
  delete fk;
}
keaki_status keaki_hip_fk_shard_sizes(const keaki_hip_fk_shard* fk, size_t* out4) {
  if (!fk || !out4) return KEAKI_ERR_BAD_ARG;
  const size_t d = (size_t)1 << fk->plan.log2d, R = fk->world;
  out4[0] = fk_shard_buffer_bytes(fk);
  out4[1] = 2 * d / R / R * 96;      // the setup's all-to-all (two d-point transforms in one exchange): bytes per peer
  out4[2] = d / R / R * 96;          // the two all-to-alls of a call (one d-point transform each)
  out4[3] = d / R * 64;              // all-gather of the affine proofs: bytes per rank
  return KEAKI_OK;
}
keaki_status keaki_hip_fk_shard_setup(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk, int32_t step, void* d_send, void* d_recv) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.fk_shard_setup");
  if (!fk || step < 0 || step > 1 || (step == 0 && !d_send) || (step == 1 && !d_recv)) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_setup: bad argument");
  // step 0 may always start over (the caller's exchange failed after it, say): it recomputes this rank's outgoing points from the SRS
  if (step != fk->setup_next && step != 0) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_setup: step %d out of order (step %d is next)", step, fk->setup_next);
  if (step == 0) { fk->plan.hat_s_ready = false; fk->setup_next = 0; }
  ST_TRY(fk_shard_setup_run(ctx, fk->plan, fk->srs->d, step, d_send, d_recv));
  fk->setup_next = step + 1;
  return KEAKI_OK;
}
keaki_status keaki_hip_fk_shard_open(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk, int32_t step, const uint64_t* coeffs, void* d_send, void* d_recv,
                                     uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.fk_shard_open");
  if (!fk || step < 0 || step > 3) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_open: bad argument");
  if (!fk->plan.hat_s_ready) return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_open: keaki_hip_fk_shard_setup steps 0 and 1 have not run");
  const size_t d = (size_t)1 << fk->plan.log2d;
  if ((step == 0 && (!coeffs || !d_send)) || (step == 1 && (!d_send || !d_recv)) || (step == 2 && (!d_send || !d_recv)) || (step == 3 && (!d_recv || !proofs_out_aff)))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_open: step %d is missing a buffer", step);
  if (step != fk->open_next && step != 0)      // step 0 may always start a new polynomial
    return fail(ctx, KEAKI_ERR_BAD_ARG, "fk_shard_open: step %d out of order (step %d is next)", step, fk->open_next);
  if (step == 0) HIP_TRY(ctx, hipMemcpyAsync(fk->plan.coeffs, coeffs, d * 32, hipMemcpyHostToDevice, ctx->stream));
  if (step < 3) {
    ST_TRY(fk_shard_open_run(ctx, fk->plan, step, d_send, d_recv, nullptr));
    fk->open_next = step + 1;
    return KEAKI_OK;
  }
  ST_TRY(reserve(ctx, ctx->io_d, d * 64));
  ST_TRY(fk_shard_open_run(ctx, fk->plan, 3, nullptr, d_recv, ctx->io_d.p));
  prefault_out(ctx, proofs_out_aff, d * 64);
  fk->open_next = 0;
  return download(ctx, proofs_out_aff, ctx->io_d.p, d * 64);
}

// ---- test hook: line table of a fixed Q (MILLER_MAX_LINES x 2 parities x 3 Fq, Montgomery)
keaki_status keaki_hip_g2_prepare(keaki_hip_ctx* ctx, const uint64_t* g2_aff, uint64_t* lines_out, size_t lines_out_bytes) {
  CTX_GUARD(ctx);
  if (!g2_aff || !lines_out || lines_out_bytes < g2_prepared_bytes()) return fail(ctx, KEAKI_ERR_BAD_ARG, "g2_prepare: bad argument");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, g2_aff, 128));
  ST_TRY(reserve(ctx, ctx->io_b, g2_prepared_bytes()));
  HIP_TRY(ctx, hipMemsetAsync(ctx->io_b.p, 0, g2_prepared_bytes(), ctx->stream));
  ST_TRY(g2_prepare_run(ctx, ctx->io_a.p, ctx->io_b.p));
  ST_TRY(reserve(ctx, ctx->io_c, g2_prepared_bytes()));
  HIP_TRY(ctx, hipMemsetAsync(ctx->io_c.p, 0, g2_prepared_bytes(), ctx->stream));
  ST_TRY(lines_to256_run(ctx, ctx->io_b.p, ctx->io_c.p));
  return download(feed, lines_out, ctx->io_c.p, g2_prepared_bytes());
}

// ---- test hook: Miller loop alone (n x 12 Fq Montgomery out)
keaki_status keaki_hip_miller_loop_batch(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, size_t n, uint64_t* f_mont_out) {
  CTX_GUARD(ctx);
  if (n == 0) return KEAKI_OK;
  if (!g1_aff || !g2_aff || !f_mont_out) return fail(ctx, KEAKI_ERR_BAD_ARG, "miller_loop_batch: null pointer");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, g1_aff, n * 64));
  ST_TRY(upload(feed, ctx->io_b, g2_aff, n * 128));
  ST_TRY(reserve(ctx, ctx->io_c, n * 384));
  ST_TRY(miller_only_run(ctx, ctx->io_a.p, ctx->io_b.p, n, ctx->io_c.p));
  return download(feed, f_mont_out, ctx->io_c.p, n * 384);
}

// ---- test hook: final exponentiation of caller-supplied Miller-loop outputs (n x 12 Fq, Montgomery) -> n x 384 GT bytes
keaki_status keaki_hip_final_exp_batch(keaki_hip_ctx* ctx, const uint64_t* f_mont, size_t n, uint8_t* gt_out) {
  CTX_GUARD(ctx);
  if (n == 0) return KEAKI_OK;
  if (!f_mont || !gt_out) return fail(ctx, KEAKI_ERR_BAD_ARG, "final_exp_batch: null pointer");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, f_mont, n * 384));
  ST_TRY(reserve(ctx, ctx->io_b, n * 384));
  ST_TRY(final_exp_only_run(ctx, ctx->io_a.p, n, ctx->io_b.p));
  return download(feed, gt_out, ctx->io_b.p, n * 384);
}

// ---- KZG open on the device (row f-4): value = p(z), proof = commit((p - p(z)) / (x - z)) ------------------------------------------
// io_c of open and quotient: [quotient nq + 1 Fr | value | work of open_quotient_run for work_n coefficients]
struct OpenLayout { size_t o_q, o_v, o_w, total; };
static OpenLayout open_layout(size_t nq, size_t work_n) {
  const size_t o_v = (nq + 1) * 32, o_w = o_v + 32;
  return {0, o_v, o_w, o_w + open_quotient_work_bytes(work_n)};
}
// one copy in front, on the context's stream: coefficients -> quotient -> MSM
static keaki_status open_resident(CopyFeed& feed, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* point, char* b, const OpenLayout& L) {
  keaki_hip_ctx* ctx = feed.ctx;
  const auto tb = srs_tables(srs);
  ST_TRY(feed.put(0, ctx->io_a.p, coeffs, n * 32));
  if (n) ST_TRY(open_quotient_run(ctx, ctx->io_a.p, n, point, b + L.o_q, b + L.o_v, b + L.o_w));
  return msm_g1_run(ctx, srs->d, srs->n, b + L.o_q, n ? n - 1 : 0, ctx->io_b.p, tb.first, tb.second);
}
// Three streams (host_plan.h: open_plan): the copy stream brings chunk j up while chunk j - 1's quotient and MSM pass run, the AUX stream
// turns it into quotient coefficients (a handful of short, latency-bound kernels that depend on the chunk above only through its carry Q_hi,
// planted as one more "coefficient" behind the chunk), the context's stream runs the MSM passes, which consume the quotient chunk by
// chunk (msm_host.hip.h: MsmPipe). The quotient of chunk j + 1 therefore runs beside the MSM pass of chunk j instead of in front of its own
// (2^24 coefficients: 20.8 -> 18.5 ms).
static keaki_status open_chunked(CopyFeed& feed, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* point, char* b, const OpenLayout& L,
                                 const OpenPlan& plan) {
  keaki_hip_ctx* ctx = feed.ctx;
  const auto tb = srs_tables(srs);
  ST_TRY(feed.begin(true));
  ST_TRY(ctx->aux.ready(ctx));
  hipStream_t ax = ctx->aux.stream, main_st = ctx->stream;
  hipEvent_t* ev = ctx->aux.open_ev;                                   // [chunk's quotient ready x 2 | start]
  HIP_TRY(ctx, hipEventRecord(ev[2], main_st));                        // behind the value slot's memset and every earlier user of io_a / io_c
  HIP_TRY(ctx, hipStreamWaitEvent(ax, ev[2], 0));
  feed.also_drain(ax);                                                 // nothing of this call is left on it at any exit
  MsmPipe pipe;
  pipe.ranges = plan.ranges;
  char* a = (char*)ctx->io_a.p;
  pipe.stage = [&](size_t j) -> keaki_status {
    const size_t lo = plan.chunks[j].first, hi = plan.chunks[j].second;
    ST_TRY(feed.put(j, a + lo * 32, (const char*)coeffs + lo * 32, (hi - lo) * 32, ax));
    {
      StreamSwap on_aux(ctx, ax);                                      // the launchers enqueue on ctx->stream
      // the carry: Q_hi = q_(hi-1), written by the chunk above; it takes the place of c_hi, which that chunk has consumed
      if (j) HIP_TRY(ctx, hipMemcpyAsync(a + hi * 32, b + L.o_q + (hi - 1) * 32, 32, hipMemcpyDeviceToDevice, ax));
      ST_TRY(open_quotient_run(ctx, a + lo * 32, hi - lo + (j ? 1 : 0), point, b + L.o_q + lo * 32, lo ? b + L.o_q + (lo - 1) * 32 : b + L.o_v, b + L.o_w, j != 0));
    }
    HIP_TRY(ctx, hipEventRecord(ev[j & 1], ax));
    HIP_TRY(ctx, hipStreamWaitEvent(main_st, ev[j & 1], 0));
    return KEAKI_OK;
  };
  return msm_g1_run(ctx, srs->d, srs->n, b + L.o_q, n - 1, ctx->io_b.p, tb.first, tb.second, &pipe);
}
keaki_status keaki_hip_kzg_open(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* point,
                                uint64_t* proof_out_jac, uint64_t* value_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_open");
  if (!srs || !point || !proof_out_jac || (n && !coeffs)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_open: null pointer");
  const size_t nq = n ? n - 1 : 0;
  ST_TRY(srs_holds(ctx, srs, "kzg_open", nq, SRS_SHORT_MSM));
  const OpenLayout L = open_layout(nq, n + 1);
  ST_TRY(reserve(ctx, ctx->io_a, n ? n * 32 : 16));
  ST_TRY(reserve(ctx, ctx->io_c, L.total));
  ST_TRY(reserve(ctx, ctx->io_b, 96));
  char* b = (char*)ctx->io_c.p;
  HIP_TRY(ctx, hipMemsetAsync(b + L.o_v, 0, 32, ctx->stream));                   // the zero polynomial evaluates to 0
  const OpenPlan plan = open_plan(ctx->tune, n);
  CopyFeed feed(ctx);
  ST_TRY(plan.chunked() ? open_chunked(feed, srs, coeffs, n, point, b, L, plan) : open_resident(feed, srs, coeffs, n, point, b, L));
  ST_TRY(download(feed, proof_out_jac, ctx->io_b.p, 96));
  if (value_out) ST_TRY(download(ctx, value_out, b + L.o_v, 32));
  resolve_timing(ctx);
  return KEAKI_OK;
}

// the quotient alone (host in / out): what keaki_hip_group_kzg_open feeds to the MSM of all members
keaki_status keaki_hip_kzg_quotient(keaki_hip_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* point, uint64_t* quotient_out,
                                    uint64_t* value_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_quotient");
  if (!point || (n && !coeffs) || (n > 1 && !quotient_out)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_quotient: null pointer");
  const size_t nq = n ? n - 1 : 0;
  const OpenLayout L = open_layout(nq, n);
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, coeffs, n * 32));
  ST_TRY(reserve(ctx, ctx->io_c, L.total));
  char* b = (char*)ctx->io_c.p;
  HIP_TRY(ctx, hipMemsetAsync(b + L.o_v, 0, 32, ctx->stream));
  if (n) ST_TRY(open_quotient_run(ctx, ctx->io_a.p, n, point, b + L.o_q, b + L.o_v, b + L.o_w));
  if (nq) HIP_TRY(ctx, hipMemcpyAsync(quotient_out, b + L.o_q, nq * 32, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, value_out, b + L.o_v, value_out ? 32 : 0);
}

// ---- KZG set openings: one proof for k points (kzg_multi.hip) -------------------------------------------------------------------------------
// ks_io: [points | values | Z | weights | I], a slot of KEAKI_SET_MAX + 1 Fr each, then [proof 96 | I1 96 | Z2 192 | com 64 | C - I1 64 | Z2 affine 128]
// ks_q:  [quotient: n Fr | work of multi_quotient_run]
namespace {
struct KsLayout {
  static constexpr size_t SLOT = ((size_t)KEAKI_SET_MAX + 1) * 32;
  static constexpr size_t O_PTS = 0, O_VAL = SLOT, O_ZC = 2 * SLOT, O_W = 3 * SLOT, O_IC = 4 * SLOT, O_PROOF = 5 * SLOT, O_I1 = O_PROOF + 96, O_Z2 = O_I1 + 96,
                          O_COM = O_Z2 + 192, O_PAIR = O_COM + 64, TOTAL = O_PAIR + 192;
};
keaki_status set_args(keaki_hip_ctx* ctx, const char* what, size_t k, bool pointers_ok) {
  if (k == 0 || k > KEAKI_SET_MAX) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: k = %zu must be in 1 .. %d", what, k, (int)KEAKI_SET_MAX);
  if (!pointers_ok) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: null pointer", what);
  return KEAKI_OK;
}
// the arguments are checked and ks_io is reserved; d_values may be null
keaki_status open_multi_core(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, const void* d_points, size_t k, void* d_proof_out_jac,
                             void* d_values) {
  using S = KsLayout;
  char* io = (char*)ctx->ks_io.p;
  ST_TRY(reserve(ctx, ctx->ks_q, n * 32 + multi_quotient_work_bytes(n)));
  char* q = (char*)ctx->ks_q.p;
  if (!d_values) d_values = io + S::O_VAL;
  ST_TRY(set_polys_run(ctx, d_points, nullptr, k, nullptr, io + S::O_W, nullptr));
  if (n == 0) HIP_TRY(ctx, hipMemsetAsync(d_values, 0, k * 32, ctx->stream));                   // the zero polynomial evaluates to 0
  // n <= k: only the values are wanted (p = I, the MSM below takes no terms); the passes still write their n - 1 quotient words, which are zero
  // and never read -- an edge case not worth a second kernel form
  else ST_TRY(multi_quotient_run(ctx, d_coeffs, n, d_points, io + S::O_W, k, q, d_values, q + n * 32));
  const auto tb = srs_tables(srs);
  return msm_g1_run(ctx, srs->d, srs->n, q, n > k ? n - 1 : 0, d_proof_out_jac, tb.first, tb.second);     // n <= k: p = I, the quotient is zero
}
}  // namespace

keaki_status keaki_hip_kzg_set_polys_dev(keaki_hip_ctx* ctx, const void* d_points, const void* d_values, size_t k, void* d_z_coeffs_out, void* d_weights_out,
                                         void* d_i_coeffs_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_set_polys");
  ST_TRY(set_args(ctx, "kzg_set_polys", k, d_points && d_z_coeffs_out && d_weights_out && (!d_i_coeffs_out || d_values)));
  return set_polys_run(ctx, d_points, d_values, k, d_z_coeffs_out, d_weights_out, d_i_coeffs_out);
}
keaki_status keaki_hip_kzg_set_polys(keaki_hip_ctx* ctx, const uint64_t* points, const uint64_t* values, size_t k, uint64_t* z_coeffs_out, uint64_t* weights_out,
                                     uint64_t* i_coeffs_out) {
  CTX_GUARD(ctx);
  using S = KsLayout;
  ST_TRY(set_args(ctx, "kzg_set_polys", k, points && z_coeffs_out && weights_out && (!i_coeffs_out || values)));
  ST_TRY(reserve(ctx, ctx->ks_io, S::TOTAL));
  char* io = (char*)ctx->ks_io.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, io + S::O_PTS, points, k * 32));
  if (i_coeffs_out) ST_TRY(feed.put(0, io + S::O_VAL, values, k * 32));
  ST_TRY(keaki_hip_kzg_set_polys_dev(ctx, io + S::O_PTS, i_coeffs_out ? io + S::O_VAL : nullptr, k, io + S::O_ZC, io + S::O_W, i_coeffs_out ? io + S::O_IC : nullptr));
  HIP_TRY(ctx, hipMemcpyAsync(z_coeffs_out, io + S::O_ZC, (k + 1) * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (i_coeffs_out) HIP_TRY(ctx, hipMemcpyAsync(i_coeffs_out, io + S::O_IC, k * 32, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, weights_out, io + S::O_W, k * 32);
}
keaki_status keaki_hip_kzg_open_multi_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, const void* d_points, size_t k,
                                          void* d_proof_out_jac, void* d_values_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_open_multi");
  ST_TRY(set_args(ctx, "kzg_open_multi", k, srs && d_points && d_proof_out_jac && (!n || d_coeffs)));
  ST_TRY(srs_holds(ctx, srs, "kzg_open_multi", n ? n - 1 : 0, SRS_SHORT_MSM));
  ST_TRY(reserve(ctx, ctx->ks_io, KsLayout::TOTAL));
  return open_multi_core(ctx, srs, d_coeffs, n, d_points, k, d_proof_out_jac, d_values_out);
}
keaki_status keaki_hip_kzg_open_multi(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* points, size_t k,
                                      uint64_t* proof_out_jac, uint64_t* values_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_open_multi");
  using S = KsLayout;
  ST_TRY(set_args(ctx, "kzg_open_multi", k, srs && points && proof_out_jac && (!n || coeffs)));
  ST_TRY(srs_holds(ctx, srs, "kzg_open_multi", n ? n - 1 : 0, SRS_SHORT_MSM));
  ST_TRY(reserve(ctx, ctx->ks_io, S::TOTAL));
  ST_TRY(reserve(ctx, ctx->io_a, n ? n * 32 : 16));
  char* io = (char*)ctx->ks_io.p;
  // one upload in front of the kernels: the chunk pipeline of keaki_hip_kzg_open is not used here
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, ctx->io_a.p, coeffs, n * 32));
  ST_TRY(feed.put(0, io + S::O_PTS, points, k * 32));
  ST_TRY(open_multi_core(ctx, srs, ctx->io_a.p, n, io + S::O_PTS, k, io + S::O_PROOF, io + S::O_VAL));
  if (values_out) HIP_TRY(ctx, hipMemcpyAsync(values_out, io + S::O_VAL, k * 32, hipMemcpyDeviceToHost, ctx->stream));
  ST_TRY(download(feed, proof_out_jac, io + S::O_PROOF, 96));
  resolve_timing(ctx);
  return KEAKI_OK;
}
keaki_status keaki_hip_kzg_aggregate_dev(keaki_hip_ctx* ctx, const void* d_points, const void* d_proofs_aff, size_t k, void* d_proof_out_jac) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_aggregate");
  using S = KsLayout;
  ST_TRY(set_args(ctx, "kzg_aggregate", k, d_points && d_proofs_aff && d_proof_out_jac));
  ST_TRY(reserve(ctx, ctx->ks_io, S::TOTAL));
  char* io = (char*)ctx->ks_io.p;
  ST_TRY(set_polys_run(ctx, d_points, nullptr, k, nullptr, io + S::O_W, nullptr));
  return msm_g1_run(ctx, d_proofs_aff, k, io + S::O_W, k, d_proof_out_jac);          // the proofs as an ad-hoc base vector: no tables
}
keaki_status keaki_hip_kzg_aggregate(keaki_hip_ctx* ctx, const uint64_t* points, const uint64_t* proofs_aff, size_t k, uint64_t* proof_out_jac) {
  CTX_GUARD(ctx);
  using S = KsLayout;
  ST_TRY(set_args(ctx, "kzg_aggregate", k, points && proofs_aff && proof_out_jac));
  ST_TRY(reserve(ctx, ctx->ks_io, S::TOTAL));
  ST_TRY(reserve(ctx, ctx->io_a, k * G1_AFF_BYTES));
  char* io = (char*)ctx->ks_io.p;
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, io + S::O_PTS, points, k * 32));
  ST_TRY(feed.put(0, ctx->io_a.p, proofs_aff, k * G1_AFF_BYTES));
  ST_TRY(keaki_hip_kzg_aggregate_dev(ctx, io + S::O_PTS, ctx->io_a.p, k, io + S::O_PROOF));
  ST_TRY(download(feed, proof_out_jac, io + S::O_PROOF, 96));
  resolve_timing(ctx);
  return KEAKI_OK;
}

// The set predicate e(C - [I(tau)]_1, g2) == e(proof, [Z(tau)]_2): the two set polynomials (kzg_multi.hip), [Z]_2 and [I]_1 by the library's MSMs over
// the powers, then keaki_hip_kzg_verify ITSELF with com := C - [I]_1, value := 0, point := 0, tau_g2 := [Z]_2 (the two points cross the host once:
// 192 bytes, which pair_out hands to the tests).
keaki_status keaki_hip_kzg_verify_multi(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                        const uint64_t* points, const uint64_t* values, size_t k, const uint64_t* proof_aff, int32_t* ok_out,
                                        uint64_t* pair_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_verify_multi");
  using S = KsLayout;
  ST_TRY(set_args(ctx, "kzg_verify_multi", k, srs_g1 && srs_g2 && com_aff && points && values && proof_aff && ok_out));
  ST_TRY(srs_holds(ctx, srs_g2, "kzg_verify_multi", k + 1, "kzg_verify_multi: Z has %zu coefficients but the G2 SRS holds %zu points"));
  ST_TRY(srs_holds(ctx, srs_g1, "kzg_verify_multi", k, "kzg_verify_multi: I has %zu coefficients but the G1 SRS holds %zu points"));
  ST_TRY(reserve(ctx, ctx->ks_io, S::TOTAL));
  char* io = (char*)ctx->ks_io.p;
  uint64_t pair[24];
  {
    CopyFeed feed(ctx);
    ST_TRY(feed.put(0, io + S::O_PTS, points, k * 32));
    ST_TRY(feed.put(0, io + S::O_VAL, values, k * 32));
    ST_TRY(feed.put(0, io + S::O_COM, com_aff, 64));
    ST_TRY(set_polys_run(ctx, io + S::O_PTS, io + S::O_VAL, k, io + S::O_ZC, io + S::O_W, io + S::O_IC));
    const auto t2 = srs_tables(srs_g2);
    ST_TRY(msm_g2_run(ctx, srs_g2->d, srs_g2->n, io + S::O_ZC, k + 1, io + S::O_Z2, t2.first, t2.second));
    const auto t1 = srs_tables(srs_g1);
    ST_TRY(msm_g1_run(ctx, srs_g1->d, srs_g1->n, io + S::O_IC, k, io + S::O_I1, t1.first, t1.second));
    ST_TRY(set_pair_points_run(ctx, io + S::O_COM, io + S::O_I1, io + S::O_Z2, io + S::O_PAIR, io + S::O_PAIR + 64));
    ST_TRY(download(feed, pair, io + S::O_PAIR, 192));
  }
  const uint64_t zero[4] = {0, 0, 0, 0};
  ST_TRY(keaki_hip_kzg_verify(ctx, pair, pair + 8, zero, zero, proof_aff, ok_out));
  if (pair_out_aff) memcpy(pair_out_aff, pair, 192);
  return KEAKI_OK;
}

// ---- batched commit / open: m rows over one SRS in one call (msm_batch.hip) ---------------------------------------------------------------
namespace {
// the argument rules the four batch entries share; *empty: m = 0, nothing to do
keaki_status batch_args(keaki_hip_ctx* ctx, const char* what, const void* srs, size_t n, size_t m, size_t stride, bool* empty) {
  *empty = false;
  if (!srs) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: srs is null", what);
  if (stride < n) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: stride %zu is shorter than a row of %zu", what, stride, n);
  if (n && m >= ((size_t)1 << 31) / n + (((size_t)1 << 31) % n ? 1 : 0)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: m * n must be < 2^31", what);
  if (m >= ((size_t)1 << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: m must be < 2^31", what);
  *empty = m == 0;
  return KEAKI_OK;
}
inline size_t batch_span(size_t n, size_t m, size_t stride) { return n && m ? ((m - 1) * stride + n) * 32 : 0; }   // bytes from row 0 to the end of row m - 1

keaki_status open_batch_core(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, size_t m, size_t stride, const void* d_points,
                             void* d_proofs_out_jac, void* d_values_out) {
  const size_t nq = n ? n - 1 : 0;
  ST_TRY(srs_holds(ctx, srs, "kzg_open_batch", nq, SRS_SHORT_MSM));
  if (n == 0 && d_values_out) HIP_TRY(ctx, hipMemsetAsync(d_values_out, 0, m * 32, ctx->stream));      // the zero polynomial evaluates to 0
  const auto tb = srs_tables(srs);
  if (nq == 0) {
    ST_TRY(fr_quotient_batch_run(ctx, d_coeffs, n, m, stride, d_points, nullptr, 0, d_values_out));
    return msm_g1_batch_run(ctx, srs->d, srs->n, tb.first, tb.second, nullptr, 0, m, 0, d_proofs_out_jac);
  }
  // the quotient rows live in a workspace, as many rows at a time as it can hold: a refused reservation halves the rows; one row is what
  // keaki_hip_kzg_open itself needs
  size_t rows = std::min(m, std::max<size_t>(1, MSM_BATCH_CANON_BYTES / (nq * 32)));
  for (;;) {
    const keaki_status st = reserve(ctx, ctx->mb_q, rows * nq * 32);
    if (st == KEAKI_OK) break;
    if (st != KEAKI_ERR_OOM || rows == 1) return st;
    ctx->err.clear();
    rows = (rows + 1) / 2;
  }
  for (size_t r0 = 0; r0 < m; r0 += rows) {
    const size_t k = std::min(rows, m - r0);
    ST_TRY(fr_quotient_batch_run(ctx, (const char*)d_coeffs + r0 * stride * 32, n, k, stride, (const char*)d_points + r0 * 32, ctx->mb_q.p, nq,
                                 d_values_out ? (char*)d_values_out + r0 * 32 : nullptr));
    ST_TRY(msm_g1_batch_run(ctx, srs->d, srs->n, tb.first, tb.second, ctx->mb_q.p, nq, k, nq, (char*)d_proofs_out_jac + r0 * G1_JAC_BYTES));
  }
  return KEAKI_OK;
}
}  // namespace

keaki_status keaki_hip_msm_g1_batch_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_scalars, size_t n, size_t m, size_t stride,
                                        void* d_out_jac) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.msm_g1_batch");
  bool empty;
  ST_TRY(batch_args(ctx, "msm_g1_batch", srs, n, m, stride, &empty));
  if (empty) return KEAKI_OK;
  if (!d_out_jac || (n && !d_scalars)) return fail(ctx, KEAKI_ERR_BAD_ARG, "msm_g1_batch: null pointer");
  ST_TRY(srs_holds(ctx, srs, "msm_g1_batch", n, SRS_SHORT_MSM));
  const auto tb = srs_tables(srs);
  return msm_g1_batch_run(ctx, srs->d, srs->n, tb.first, tb.second, d_scalars, n, m, stride, d_out_jac);
}
keaki_status keaki_hip_msm_g1_batch(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* scalars, size_t n, size_t m, size_t stride,
                                    uint64_t* out_jac) {
  CTX_GUARD(ctx);
  bool empty;
  ST_TRY(batch_args(ctx, "msm_g1_batch", srs, n, m, stride, &empty));
  if (empty) return KEAKI_OK;
  if (!out_jac || (n && !scalars)) return fail(ctx, KEAKI_ERR_BAD_ARG, "msm_g1_batch: null pointer");
  ST_TRY(srs_holds(ctx, srs, "msm_g1_batch", n, SRS_SHORT_MSM));
  // one upload in front, the kernels, one download of m x 96 B: the rows are short, there is nothing for a chunk pipeline to hide
  ST_TRY(reserve(ctx, ctx->io_b, m * G1_JAC_BYTES));
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, scalars, batch_span(n, m, stride)));
  ST_TRY(keaki_hip_msm_g1_batch_dev(ctx, srs, ctx->io_a.p, n, m, stride, ctx->io_b.p));
  prefault_out(ctx, out_jac, m * G1_JAC_BYTES);
  return download(feed, out_jac, ctx->io_b.p, m * G1_JAC_BYTES);
}
keaki_status keaki_hip_kzg_open_batch_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, size_t m, size_t stride,
                                          const void* d_points, void* d_proofs_out_jac, void* d_values_out) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.kzg_open_batch");
  bool empty;
  ST_TRY(batch_args(ctx, "kzg_open_batch", srs, n, m, stride, &empty));
  if (empty) return KEAKI_OK;
  if (!d_points || !d_proofs_out_jac || (n && !d_coeffs)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_open_batch: null pointer");
  return open_batch_core(ctx, srs, d_coeffs, n, m, stride, d_points, d_proofs_out_jac, d_values_out);
}
keaki_status keaki_hip_kzg_open_batch(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, size_t m, size_t stride,
                                      const uint64_t* points, uint64_t* proofs_out_jac, uint64_t* values_out) {
  CTX_GUARD(ctx);
  bool empty;
  ST_TRY(batch_args(ctx, "kzg_open_batch", srs, n, m, stride, &empty));
  if (empty) return KEAKI_OK;
  if (!points || !proofs_out_jac || (n && !coeffs)) return fail(ctx, KEAKI_ERR_BAD_ARG, "kzg_open_batch: null pointer");
  ST_TRY(srs_holds(ctx, srs, "kzg_open_batch", n ? n - 1 : 0, SRS_SHORT_MSM));
  ST_TRY(reserve(ctx, ctx->io_b, m * G1_JAC_BYTES));
  ST_TRY(reserve(ctx, ctx->io_d, m * 32));
  ST_TRY(reserve(ctx, ctx->io_a, std::max<size_t>(16, batch_span(n, m, stride))));
  ST_TRY(reserve(ctx, ctx->io_c, m * 32));
  CopyFeed feed(ctx);
  ST_TRY(feed.put(0, ctx->io_a.p, coeffs, batch_span(n, m, stride)));
  ST_TRY(feed.put(0, ctx->io_c.p, points, m * 32));
  ST_TRY(keaki_hip_kzg_open_batch_dev(ctx, srs, ctx->io_a.p, n, m, stride, ctx->io_c.p, ctx->io_b.p, ctx->io_d.p));
  if (values_out) HIP_TRY(ctx, hipMemcpyAsync(values_out, ctx->io_d.p, m * 32, hipMemcpyDeviceToHost, ctx->stream));
  return download(feed, proofs_out_jac, ctx->io_b.p, m * G1_JAC_BYTES);
}

// ---- batched FK23 openings / vec_commit: m rows over one domain in one call (fk_batch.hip) --------------------------------------------------
namespace {
// the domain constants of a call (host pointers, read before the call returns); omega_d_inv / inv_d: vec_commit only
struct FkbConsts { const uint64_t *omega_d_inv, *inv_d, *omega_2d, *omega_2d_inv, *inv_2d; };
// How the four entries start: fk_enter, then the row layout. n: elements read of a row (d for open_fk_poly_batch). *empty: m = 0.
keaki_status fkb_enter(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, bool ptrs_ok, const char* what, size_t n, size_t m, size_t stride,
                       std::unique_lock<std::recursive_mutex>& hl, bool* empty) {
  *empty = false;
  ST_TRY(fk_enter(ctx, srs, log2d, ptrs_ok || m == 0, what, hl));
  const size_t d = (size_t)1 << log2d;
  if (n > d) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: %zu evaluations do not fit the domain of %zu", what, n, d);
  if (stride < n) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: stride %zu is shorter than a row of %zu", what, stride, n);
  if (m >= ((size_t)1 << (31 - log2d))) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: m * d must be < 2^31", what);
  *empty = m == 0;
  return KEAKI_OK;
}
// row by row through the single pipeline (device rows): the steps of keaki_hip_open_fk_poly / keaki_hip_vec_commit between their copies
keaki_status fkb_row_single(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_row, size_t n, const FkbConsts& k, void* d_com, void* d_proofs) {
  const size_t d = (size_t)1 << log2d;
  const size_t o_c = 0, o_tw = o_c + d * 32, o_fr = o_tw + (d / 2 + 1) * 32, o_g = o_fr + open_fk_poly_fr_bytes(log2d), total = o_g + open_fk_poly_g_bytes(log2d);
  ST_TRY(reserve(ctx, ctx->io_d, total));
  char* b = (char*)ctx->io_d.p;
  if (!d_com) return open_fk_from_poly(ctx, srs, log2d, d_row, k.omega_2d, k.omega_2d_inv, k.inv_2d, b + o_fr, b + o_g, d_proofs);
  if (n < d) HIP_TRY(ctx, hipMemsetAsync(b + o_c + n * 32, 0, (d - n) * 32, ctx->stream));
  if (n) HIP_TRY(ctx, hipMemcpyAsync(b + o_c, d_row, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
  ST_TRY(fr_fft_run(ctx, b + o_c, log2d, k.omega_d_inv, k.inv_d, b + o_tw));
  ST_TRY(open_fk_from_poly(ctx, srs, log2d, b + o_c, k.omega_2d, k.omega_2d_inv, k.inv_2d, b + o_fr, b + o_g, d_proofs));
  const auto tb = srs_tables(srs);
  return msm_g1_run(ctx, srs->d, srs->n, b + o_c, d, d_com, tb.first, tb.second);
}
// d_com == null: open_fk_poly_batch (rows of d coefficients); else vec_commit_batch (rows of n evaluations). Everything on the device.
keaki_status fkb_core(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_rows, size_t n, size_t m, size_t stride, const FkbConsts& k,
                      void* d_com, void* d_proofs) {
  const size_t d = (size_t)1 << log2d;
  // the pass: as many rows as the cap allows; a refused reservation halves it, a refused single row sends the call through the single pipeline
  size_t rows = 0;
  if (log2d >= 1 && log2d <= FKB_LOG2D_MAX) {
    rows = fkb_rows_per_pass(log2d, m);
    for (;;) {
      const keaki_status st = fkb_reserve(ctx, log2d, rows);
      if (st == KEAKI_OK) break;
      if (st != KEAKI_ERR_OOM) return st;
      ctx->err.clear();
      if (rows == 1) { rows = 0; break; }
      rows = (rows + 1) / 2;
    }
  }
  if (rows == 0) {
    for (size_t j = 0; j < m; j++)
      ST_TRY(fkb_row_single(ctx, srs, log2d, (const char*)d_rows + j * stride * 32, n, k, d_com ? (char*)d_com + j * G1_JAC_BYTES : nullptr,
                            (char*)d_proofs + j * d * G1_AFF_BYTES));
    return KEAKI_OK;
  }
  const void* tw = fkb_tables_run(ctx, log2d, rows, k.omega_2d, k.omega_2d_inv, d_com ? k.omega_d_inv : nullptr);
  ST_TRY(fk_cache_ensure(ctx, srs, log2d, tw));
  const auto tb = srs_tables(srs);
  for (size_t r0 = 0; r0 < m; r0 += rows) {
    const size_t cnt = std::min(rows, m - r0);
    const void* coeffs = nullptr;
    ST_TRY(fkb_pass_run(ctx, srs->fk.p, log2d, rows, (const char*)d_rows + r0 * stride * 32, n, (uint32_t)cnt, stride, d_com ? k.inv_d : nullptr, k.inv_2d,
                        (char*)d_proofs + r0 * d * G1_AFF_BYTES, &coeffs));
    if (d_com) ST_TRY(msm_g1_batch_run(ctx, srs->d, srs->n, tb.first, tb.second, coeffs, d, cnt, d, (char*)d_com + r0 * G1_JAC_BYTES));
  }
  return KEAKI_OK;
}
}  // namespace

keaki_status keaki_hip_open_fk_poly_batch_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_coeffs, size_t m, size_t stride,
                                              const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d, void* d_proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.open_fk_batch");
  std::unique_lock<std::recursive_mutex> hl;
  bool empty;
  ST_TRY(fkb_enter(ctx, srs, log2d, d_coeffs && omega_2d && omega_2d_inv && inv_2d && d_proofs_out_aff, "open_fk_poly_batch", (size_t)1 << std::min(log2d, 27u), m, stride, hl, &empty));
  if (empty) return KEAKI_OK;
  return fkb_core(ctx, srs, log2d, d_coeffs, (size_t)1 << log2d, m, stride, {nullptr, nullptr, omega_2d, omega_2d_inv, inv_2d}, nullptr, d_proofs_out_aff);
}
keaki_status keaki_hip_open_fk_poly_batch(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* coeffs, size_t m, size_t stride,
                                          const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  std::unique_lock<std::recursive_mutex> hl;
  bool empty;
  ST_TRY(fkb_enter(ctx, srs, log2d, coeffs && omega_2d && omega_2d_inv && inv_2d && proofs_out_aff, "open_fk_poly_batch", (size_t)1 << std::min(log2d, 27u), m, stride, hl, &empty));
  if (empty) return KEAKI_OK;
  // one upload of the rows in front, the kernels, one download: the rows are short, there is nothing for a chunk pipeline to hide
  const size_t d = (size_t)1 << log2d, out_bytes = m * d * G1_AFF_BYTES;
  ST_TRY(reserve(ctx, ctx->io_b, out_bytes));
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, coeffs, batch_span(d, m, stride)));
  ST_TRY(keaki_hip_open_fk_poly_batch_dev(ctx, srs, log2d, ctx->io_a.p, m, stride, omega_2d, omega_2d_inv, inv_2d, ctx->io_b.p));
  prefault_out(ctx, proofs_out_aff, out_bytes);
  return download(feed, proofs_out_aff, ctx->io_b.p, out_bytes);
}
keaki_status keaki_hip_vec_commit_batch_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const void* d_evals, size_t n, size_t m, size_t stride, uint32_t log2d,
                                            const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                                            const uint64_t* inv_2d, void* d_com_out_jac, void* d_proofs_out_aff) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.vec_commit_batch");
  std::unique_lock<std::recursive_mutex> hl;
  bool empty;
  ST_TRY(fkb_enter(ctx, srs, log2d, (!n || d_evals) && omega_d_inv && inv_d && omega_2d && omega_2d_inv && inv_2d && d_com_out_jac && d_proofs_out_aff,
                   "vec_commit_batch", n, m, stride, hl, &empty));
  if (empty) return KEAKI_OK;
  return fkb_core(ctx, srs, log2d, d_evals, n, m, stride, {omega_d_inv, inv_d, omega_2d, omega_2d_inv, inv_2d}, d_com_out_jac, d_proofs_out_aff);
}
keaki_status keaki_hip_vec_commit_batch(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const uint64_t* evals, size_t n, size_t m, size_t stride, uint32_t log2d,
                                        const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                                        const uint64_t* inv_2d, uint64_t* com_out_jac, uint64_t* proofs_out_aff) {
  CTX_GUARD(ctx);
  std::unique_lock<std::recursive_mutex> hl;
  bool empty;
  ST_TRY(fkb_enter(ctx, srs, log2d, (!n || evals) && omega_d_inv && inv_d && omega_2d && omega_2d_inv && inv_2d && com_out_jac && proofs_out_aff,
                   "vec_commit_batch", n, m, stride, hl, &empty));
  if (empty) return KEAKI_OK;
  const size_t d = (size_t)1 << log2d, out_bytes = m * d * G1_AFF_BYTES;
  ST_TRY(reserve(ctx, ctx->io_b, out_bytes));
  ST_TRY(reserve(ctx, ctx->io_c, m * G1_JAC_BYTES));
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, evals, batch_span(n, m, stride)));
  ST_TRY(keaki_hip_vec_commit_batch_dev(ctx, srs, ctx->io_a.p, n, m, stride, log2d, omega_d_inv, inv_d, omega_2d, omega_2d_inv, inv_2d, ctx->io_c.p, ctx->io_b.p));
  prefault_out(ctx, proofs_out_aff, out_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(com_out_jac, ctx->io_c.p, m * G1_JAC_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  ST_TRY(download(feed, proofs_out_aff, ctx->io_b.p, out_bytes));
  resolve_timing(ctx);
  return KEAKI_OK;
}

// ---- SRS ingest: on-curve check (row f-3) ------------------------------------------------------------------------
// The tally of the calls that count in io_e (the curve check, the codec): the 16-byte slot is reserved, then begun (api_host.h: BadTally).
static keaki_status io_e_tally_begin(keaki_hip_ctx* ctx) {
  ST_TRY(reserve(ctx, ctx->io_e, 16));
  return BadTally{ctx, ctx->io_e.p}.begin();
}
static keaki_status curve_check_common(keaki_hip_ctx* ctx, bool g2, const void* d_pts, size_t n, uint64_t* n_off_curve, uint64_t* first_off_curve) {
  ST_TRY(io_e_tally_begin(ctx));
  if (n) ST_TRY(g2 ? g2_curve_check_run(ctx, d_pts, n, ctx->io_e.p) : g1_curve_check_run(ctx, d_pts, n, ctx->io_e.p));
  return BadTally{ctx, ctx->io_e.p}.end(n_off_curve, first_off_curve);
}
keaki_status keaki_hip_srs_g1_check(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, uint64_t* n_off_curve, uint64_t* first_off_curve) {
  CTX_GUARD(ctx);
  if (!srs || !n_off_curve) return fail(ctx, KEAKI_ERR_BAD_ARG, "srs_g1_check: null pointer");
  return curve_check_common(ctx, false, srs->d, srs->n, n_off_curve, first_off_curve);
}
keaki_status keaki_hip_g2_check(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint64_t* n_off_curve, uint64_t* first_off_curve) {
  CTX_GUARD(ctx);
  if (!n_off_curve || (n && !points_aff)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g2_check: null pointer");
  CopyFeed feed(ctx);
  ST_TRY(upload(feed, ctx->io_a, points_aff, n * 128));
  return feed.closed_by(curve_check_common(ctx, true, ctx->io_a.p, n, n_off_curve, first_off_curve));      // which has downloaded the counters
}

// ---- compressed point wire format (point_codec.hip): compress, decompress with validation, G2 subgroup check --------------------------------
// Rejected items are counted on the device: io_e = {count, first index}, added to by every launch of a call (the host forms run in chunks and
// pass each chunk's first index). Host forms go through the stager of the KEM host batches (pipelined_regions); from PIPE_CHUNK items on that is
// a pipeline of two halves, then of PIPE_CHUNK-item chunks.
namespace {
struct CodecGroup { bool g2; size_t aff, wire; const char* name; };
constexpr CodecGroup CODEC_G1 = {false, G1_AFF_BYTES, 32, "g1"}, CODEC_G2 = {true, G2_AFF_BYTES, 64, "g2"};
size_t codec_chunk_items(const keaki_hip_ctx* ctx, size_t n) {
  if (!ctx->tune.pipe_chunks || n < PIPE_CHUNK) return n;
  return n >= 2 * PIPE_CHUNK ? PIPE_CHUNK : (((n + 1) / 2 + 63) & ~(size_t)63);
}
keaki_status codec_n_check(keaki_hip_ctx* ctx, const char* what, size_t n) {
  if (n >= (1ull << 31)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s: n must be < 2^31 per call", what);
  return KEAKI_OK;
}
keaki_status compress_dev(const CodecGroup& g, keaki_hip_ctx* ctx, const void* d_points, size_t n, void* d_bytes) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.point_compress");
  if (n && (!d_points || !d_bytes)) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_compress: null pointer", g.name);
  ST_TRY(codec_n_check(ctx, "compress", n));
  return point_compress_run(ctx, g.g2, d_points, n, d_bytes);
}
keaki_status compress_host(const CodecGroup& g, keaki_hip_ctx* ctx, const uint64_t* points, size_t n, uint8_t* bytes) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.point_compress");
  if (n == 0) return KEAKI_OK;
  if (!points || !bytes) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_compress: null pointer", g.name);
  ST_TRY(codec_n_check(ctx, "compress", n));
  return pipelined_regions(ctx, n, codec_chunk_items(ctx, n), {}, {{points, nullptr, g.aff}, {nullptr, bytes, g.wire}},
    [&](size_t, size_t m, char* const*, char* const* d) { return point_compress_run(ctx, g.g2, d[0], m, d[1]); });
}
keaki_status decompress_args(const CodecGroup& g, keaki_hip_ctx* ctx, const void* bytes, size_t n, int32_t check_subgroup, const void* out, uint64_t* n_bad) {
  if (check_subgroup != 0 && check_subgroup != 1) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_decompress: check_subgroup = %d: must be 0 or 1", g.name, (int)check_subgroup);
  if (!n_bad || (n && (!bytes || !out))) return fail(ctx, KEAKI_ERR_BAD_ARG, "%s_decompress: null pointer", g.name);
  return codec_n_check(ctx, "decompress", n);
}
// the kernels of items [lo, lo + m)
keaki_status decompress_run(const CodecGroup& g, keaki_hip_ctx* ctx, const void* d_bytes, size_t lo, size_t m, bool check_subgroup, void* d_out, void* d_status) {
  ST_TRY(point_decompress_run(ctx, g.g2, d_bytes, m, lo, d_out, d_status, ctx->io_e.p));
  if (g.g2 && check_subgroup) ST_TRY(g2_subgroup_run(ctx, d_out, m, lo, d_status, true, ctx->io_e.p));
  return KEAKI_OK;
}
keaki_status decompress_dev(const CodecGroup& g, keaki_hip_ctx* ctx, const void* d_bytes, size_t n, int32_t check_subgroup, void* d_out, void* d_status,
                            uint64_t* n_bad, uint64_t* first_bad) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.point_decompress");
  ST_TRY(decompress_args(g, ctx, d_bytes, n, check_subgroup, d_out, n_bad));
  ST_TRY(io_e_tally_begin(ctx));
  ST_TRY(decompress_run(g, ctx, d_bytes, 0, n, check_subgroup != 0, d_out, d_status));
  return BadTally{ctx, ctx->io_e.p}.end(n_bad, first_bad);
}
keaki_status decompress_host(const CodecGroup& g, keaki_hip_ctx* ctx, const uint8_t* bytes, size_t n, int32_t check_subgroup, uint64_t* out, uint8_t* status,
                             uint64_t* n_bad, uint64_t* first_bad) {
  CTX_GUARD(ctx);                 // one lock from staging to the last download: io_a and io_e belong to this call until it returns
  TRACE_SCOPE("keaki.point_decompress");
  ST_TRY(decompress_args(g, ctx, bytes, n, check_subgroup, out, n_bad));
  ST_TRY(io_e_tally_begin(ctx));
  if (n)                          // the status bytes come last: every other region is a multiple of 16 B per item, so all of them stay aligned
                                  // status == NULL: a region with neither `in` nor `out` is device scratch of the stager, so the kernels still get a valid
                                  // d_status (they write it, nothing downloads it) -- never a null pointer, never a copy to NULL
    ST_TRY(pipelined_regions(ctx, n, codec_chunk_items(ctx, n), {}, {{bytes, nullptr, g.wire}, {nullptr, out, g.aff}, {nullptr, status, 1}},
      [&](size_t lo, size_t m, char* const*, char* const* d) { return decompress_run(g, ctx, d[0], lo, m, check_subgroup != 0, d[1], d[2]); }));
  return BadTally{ctx, ctx->io_e.p}.end(n_bad, first_bad);
}
}  // namespace

keaki_status keaki_hip_g1_compress(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint8_t* bytes_out) { return compress_host(CODEC_G1, ctx, points_aff, n, bytes_out); }
keaki_status keaki_hip_g2_compress(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint8_t* bytes_out) { return compress_host(CODEC_G2, ctx, points_aff, n, bytes_out); }
keaki_status keaki_hip_g1_compress_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, void* d_bytes_out) { return compress_dev(CODEC_G1, ctx, d_points_aff, n, d_bytes_out); }
keaki_status keaki_hip_g2_compress_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, void* d_bytes_out) { return compress_dev(CODEC_G2, ctx, d_points_aff, n, d_bytes_out); }
keaki_status keaki_hip_g1_decompress(keaki_hip_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_aff, uint8_t* status, uint64_t* n_bad, uint64_t* first_bad) {
  return decompress_host(CODEC_G1, ctx, bytes, n, 0, out_aff, status, n_bad, first_bad);
}
keaki_status keaki_hip_g2_decompress(keaki_hip_ctx* ctx, const uint8_t* bytes, size_t n, int32_t check_subgroup, uint64_t* out_aff, uint8_t* status,
                                     uint64_t* n_bad, uint64_t* first_bad) {
  return decompress_host(CODEC_G2, ctx, bytes, n, check_subgroup, out_aff, status, n_bad, first_bad);
}
keaki_status keaki_hip_g1_decompress_dev(keaki_hip_ctx* ctx, const void* d_bytes, size_t n, void* d_out_aff, void* d_status, uint64_t* n_bad, uint64_t* first_bad) {
  return decompress_dev(CODEC_G1, ctx, d_bytes, n, 0, d_out_aff, d_status, n_bad, first_bad);
}
keaki_status keaki_hip_g2_decompress_dev(keaki_hip_ctx* ctx, const void* d_bytes, size_t n, int32_t check_subgroup, void* d_out_aff, void* d_status,
                                         uint64_t* n_bad, uint64_t* first_bad) {
  return decompress_dev(CODEC_G2, ctx, d_bytes, n, check_subgroup, d_out_aff, d_status, n_bad, first_bad);
}
keaki_status keaki_hip_g2_subgroup_check_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, uint64_t* n_outside, uint64_t* first_outside) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.g2_subgroup_check");
  if (!n_outside || (n && !d_points_aff)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g2_subgroup_check: null pointer");
  ST_TRY(codec_n_check(ctx, "g2_subgroup_check", n));
  ST_TRY(io_e_tally_begin(ctx));
  ST_TRY(g2_subgroup_run(ctx, const_cast<void*>(d_points_aff), n, 0, nullptr, false, ctx->io_e.p));     // clear = false: the points are only read
  return BadTally{ctx, ctx->io_e.p}.end(n_outside, first_outside);
}
keaki_status keaki_hip_g2_subgroup_check(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint64_t* n_outside, uint64_t* first_outside) {
  CTX_GUARD(ctx);
  TRACE_SCOPE("keaki.g2_subgroup_check");
  if (!n_outside || (n && !points_aff)) return fail(ctx, KEAKI_ERR_BAD_ARG, "g2_subgroup_check: null pointer");
  ST_TRY(codec_n_check(ctx, "g2_subgroup_check", n));
  ST_TRY(io_e_tally_begin(ctx));
  if (n)
    ST_TRY(pipelined_regions(ctx, n, codec_chunk_items(ctx, n), {}, {{points_aff, nullptr, G2_AFF_BYTES}},
      [&](size_t lo, size_t m, char* const*, char* const* d) { return g2_subgroup_run(ctx, d[0], m, lo, nullptr, false, ctx->io_e.p); }));
  return BadTally{ctx, ctx->io_e.p}.end(n_outside, first_outside);
}

// ---- self-test --------------------------------------------------------------------------------------------
keaki_status keaki_hip_selftest_field(keaki_hip_ctx* ctx, uint32_t blocks, uint32_t iters, uint32_t seed, uint64_t* mismatches_out) {
  CTX_GUARD(ctx);
  if (!mismatches_out || blocks == 0) return fail(ctx, KEAKI_ERR_BAD_ARG, "selftest_field: bad argument");
  ST_TRY(reserve(ctx, ctx->io_e, 16));
  HIP_TRY(ctx, hipMemsetAsync(ctx->io_e.p, 0, 8, ctx->stream));
  ST_TRY(selftest_field_run(ctx, blocks, iters, seed, ctx->io_e.p));
  return download(ctx, mismatches_out, ctx->io_e.p, 8);
}
keaki_status keaki_hip_selftest_field_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out) {
  CTX_GUARD(ctx);
  if (!operands || !out || op >= KEAKI_FOP_COUNT || n == 0 || n > KEAKI_FOP_MAX_RECORDS || (field_probe_is_pair(op) && (n & 1)))
    return fail(ctx, KEAKI_ERR_BAD_ARG, "selftest_field_ops: bad argument");
  const size_t rec = (size_t)KEAKI_FOP_SLOTS * KEAKI_FOP_SLOT_WORDS * 4, padded = field_probe_padded(op, n);
  CopyFeed feed(ctx);
  ST_TRY(reserve(ctx, ctx->io_a, padded * rec));
  ST_TRY(reserve(ctx, ctx->io_b, n * KEAKI_FOP_SLOT_WORDS * 4));
  ST_TRY(feed.put(0, ctx->io_a.p, operands, n * rec));
  for (size_t i = n; i < padded; i++) ST_TRY(feed.put(0, (char*)ctx->io_a.p + i * rec, operands, rec));     // the tail lanes of a lane-pair op run record 0
  ST_TRY(field_probe_run(ctx, op, ctx->io_a.p, n, ctx->io_b.p));
  return download(feed, out, ctx->io_b.p, n * KEAKI_FOP_SLOT_WORDS * 4);
}
keaki_status keaki_hip_selftest_tower_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out) {
  CTX_GUARD(ctx);
  if (!operands || !out || op >= KEAKI_TOP_COUNT || n == 0 || n > KEAKI_TOP_MAX_RECORDS)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "selftest_tower_ops: bad argument");
  const size_t rec = (size_t)KEAKI_TOP_REC_WORDS * 4, padded = tower_probe_padded(op, n);
  CopyFeed feed(ctx);
  ST_TRY(reserve(ctx, ctx->io_a, padded * rec));
  ST_TRY(reserve(ctx, ctx->io_b, n * KEAKI_TOP_OUT_WORDS * 4));
  ST_TRY(feed.put(0, ctx->io_a.p, operands, n * rec));
  for (size_t i = n; i < padded; i++) ST_TRY(feed.put(0, (char*)ctx->io_a.p + i * rec, operands, rec));     // the tail lanes of a wave run record 0
  ST_TRY(tower_probe_run(ctx, op, ctx->io_a.p, n, ctx->io_b.p));
  return download(feed, out, ctx->io_b.p, n * KEAKI_TOP_OUT_WORDS * 4);
}
keaki_status keaki_hip_selftest_point_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out) {
  CTX_GUARD(ctx);
  if (!operands || !out || op >= KEAKI_POP_COUNT || n == 0 || n > KEAKI_POP_MAX_RECORDS)
    return fail(ctx, KEAKI_ERR_BAD_ARG, "selftest_point_ops: bad argument");
  const size_t rec = (size_t)KEAKI_POP_SLOTS * KEAKI_POP_SLOT_WORDS * 4, orec = (size_t)KEAKI_POP_OUT_SLOTS * KEAKI_POP_SLOT_WORDS * 4;
  const size_t padded = point_probe_padded(n), tab = point_probe_table_bytes(op, n);
  CopyFeed feed(ctx);
  ST_TRY(reserve(ctx, ctx->io_a, padded * rec));
  ST_TRY(reserve(ctx, ctx->io_b, padded * orec));          // every lane that runs has a record; the first n come back
  if (tab) ST_TRY(reserve(ctx, ctx->fk_tab, tab));
  ST_TRY(feed.put(0, ctx->io_a.p, operands, n * rec));
  for (size_t i = n; i < padded; i++) ST_TRY(feed.put(0, (char*)ctx->io_a.p + i * rec, operands, rec));     // the tail lanes of a wave run record 0
  HIP_TRY(ctx, hipMemsetAsync(ctx->io_b.p, 0, padded * orec, ctx->stream));
  ST_TRY(point_probe_run(ctx, op, ctx->io_a.p, n, ctx->io_b.p, tab ? ctx->fk_tab.p : nullptr));
  return download(feed, out, ctx->io_b.p, n * orec);
}
