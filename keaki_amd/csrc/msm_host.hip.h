// Host-side driver of the MSM pipeline (workspace sizing, window choice, kernel sequence), written
// once and instantiated for G1 (msm_g1.hip) and G2 (msm_g2.hip).
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>
#include "internal.h"
#include "msm.hip.h"

namespace keaki_internal {
using namespace bn254;

// GPU window choice: minimise (n * W mixed adds) + (2 * W * B full adds, ~1.4x a mixed add each)
// while keeping enough buckets (= lanes of the accumulate kernel) to fill 256 CUs.
inline int choose_window(size_t n, int forced = 0) {
  if (forced >= 3 && forced <= 24) return forced;         // Tuning::msm_c
  if (n < 32) return 3;
  double best = 1e300;
  int bc = 3;
  for (int c = 3; c <= 22; c++) {
    MsmPlan p = msm_make_plan(n, c);
    if (p.nb > ((size_t)PART_MAX_BINS << PART_MAX_FINE_SHIFT)) continue;      // the two-pass partition addresses 2048 x 2048 buckets
    double cost = (double)n * p.s.W + 2.8 * (double)p.nb;
    if ((double)p.nb < 131072.0) cost *= 131072.0 / (double)p.nb;   // too few buckets cannot fill 256 CUs
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}

// smallest shared window (buckets) that automatic selection reduces by row and column sums; at least 2^ROWCOL_MIN_CR (one tile)
constexpr u32 ROWCOL_MIN_B = 1u << 12;
static_assert(ROWCOL_MIN_B >= (1u << ROWCOL_MIN_CR), "k_msm_rowcol needs one 64 x 64 tile");
static_assert(16 * IDXQ_NQ == 64, "w_sorted is padded by one aligned group of the index stream: the 64 bytes segq_fetch reads");

// Everything one MSM call decides before its first launch (msm_plan_call; tests/variant_cases.py restates these rules in Python)
struct MsmCall {
  struct Pass {                    // one for a resident scalar vector, one per chunk of a pipelined call
    size_t lo, m, pairs, max_chunks, cm_bytes, bt_bytes, bm_bytes, sg_bytes, ts_bytes;
    PartShape ps;
  };
  bool shared, rowcol;             // window tables: all windows share one bucket set | tail by row and column sums (else running sums)
  bool u29, lazy_state;            // what the call WANTS: the 29-bit bucket kernel | its registers parked in Acc29 between the passes
  MsmShape s, rs;                  // shape of the passes (stride set on the shared path) | of the reduction
  size_t nb, rc_points;            // buckets the passes fill | points of the row / column tail's workspace
  u32 max_b, L, chunks;            // largest window's buckets | chunk length and chunks per window of k_msm_reduce
  std::vector<Pass> passes;
  size_t w_digits = 0, w_sorted = 0, w_offsets = 0, w_cursor = 0, w_pairs = 0;      // workspace sizes: the largest pass's
  u32 hv_cap, hv_slice_cap;        // heavy-bucket list: [bucket[cap] | first[cap] | owner[slice_cap]] (hv_hdr bytes) then the slice sums
  size_t hv_hdr = 0;
  char msg[160];                   // why the call is refused (the status is msm_plan_call's return value)
};

// The plan of one call from the tuning, the sizes and the chunk ranges alone: no HIP call, no context. d_table != nullptr is `has_table`
// (tables built by msm_build_tables with window target c_table for N = srs_len points); ranges: MsmPipe::ranges, null = one resident pass.
template <class F>
keaki_status msm_plan_call(const Tuning& t, size_t n, size_t srs_len, bool has_table, int c_table,
                           const std::vector<std::pair<size_t, size_t>>* ranges, MsmCall& c) {
#define MSM_REFUSE(code, ...) do { snprintf(c.msg, sizeof c.msg, __VA_ARGS__); return code; } while (0)
  if (n > srs_len) MSM_REFUSE(KEAKI_ERR_TOO_LARGE, "msm: %zu scalars but the SRS holds %zu points", n, srs_len);
  if (n >= (1ull << 31)) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: n must be < 2^31 per device");
  // An SRS with window tables uses them for EVERY length. Until round 4 a polynomial shorter than half of the SRS took the generic path ("its own
  // window size is faster"): true for the additions, but the generic tail is a chain of ~250 doublings and W additions in one lane -- 1.8-2.3 ms
  // whatever n is, against 0.4-0.7 ms for the one shared window (bench_tools/ab_short_msm.py: SRS 2^10 ... 2^24, n = 1 ... srs/2: the tables win
  // every cell, 3-5 x at the lengths of BASELINE config 1). Option msm_short_tables = 0 brings the old rule back (A/B, tests).
  c.shared = has_table && (n * 2 > srs_len || t.msm_short_tables != 0);
  const MsmPlan plan = c.shared ? msm_make_plan(n, c_table) : msm_make_plan(n, choose_window(n, t.msm_c));
  // reduction shape: generic = the plan itself; shared = ONE window holding max_b = 2^cr buckets (top-window rule: 2^width buckets)
  c.s = c.rs = plan.s; c.nb = plan.nb; c.max_b = plan.max_b;
  if (c.shared) {
    c.s.stride = (u32)srs_len;
    u32 cr = 0;
    while ((1u << cr) < plan.max_b) cr++;
    c.rs.c = cr; c.rs.W = 1; c.rs.k = 1;
    c.nb = plan.max_b;
    if ((double)srs_len * c.s.W >= 2147483647.0) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: precomputed table index overflows 31 bits");
  }
  if ((double)n * c.s.W >= 4294967295.0) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: n * windows overflows 32-bit positions");
  // bucket reduction. reduce_l == 0 (automatic): one shared window of at least ROWCOL_MIN_B buckets is reduced by row and column sums
  // (k_msm_rowcol*), everything else by the chunked running sums (k_msm_reduce) with the chunk length L below; reduce_l >= 1 forces the running
  // sums with that L. A lane of k_msm_reduce is a serial chain of 2 L additions plus a double-and-add by the chunk index (up to 2 log2(B / L)
  // more), so L trades chain length against the number of lanes; measured (bench_tools/sweep_reduce_l.py, round 3, whole MSM with tables):
  // 2^21 buckets (2^23, 2^24 points): 32 -- 9.42 / 17.69 ms against 9.60 / 17.88 with 16; 2^19 buckets (2^21, 2^22 points): 8 -- 2.92 /
  // 5.31 ms against 2.99 / 5.41; 16 in between; 8 below
  // (G2, whose additions cost 2.3 x as much: 8 from 2^19 buckets on as well -- 5.10 vs 5.34 ms at 2^20 points)
  c.L = sizeof(F) > sizeof(Fq) ? (plan.max_b >= 64 ? 8 : plan.max_b)
                               : plan.max_b >= (1u << 21) ? 32 : plan.max_b >= (1u << 20) ? 16 : (plan.max_b >= 64 ? 8 : plan.max_b);
  if (t.reduce_l >= 1 && t.reduce_l <= 4096 && (u32)t.reduce_l <= plan.max_b) c.L = (u32)t.reduce_l;
  c.chunks = cdiv(plan.max_b, c.L);
  c.rowcol = t.reduce_l == 0 && c.rs.W == 1 && plan.max_b >= ROWCOL_MIN_B;
  // row / column tail: per-tile sums (2 per 64 buckets), the 2^k + 2^(cr-k) sums, the cr + 1 plane terms
  c.rc_points = c.rowcol ? (size_t)plan.max_b / 32 + 2 * ((size_t)1 << ((c.rs.c + 1) / 2)) + 32 : 0;
  if (n == 0) return KEAKI_OK;                 // no pass: msm_dev writes the identity
  // ---- the passes: one for a resident scalar vector, one per chunk of a pipelined call ----------------------------------------------
  const size_t K = ranges ? ranges->size() : 1;
  if (ranges && K < 1) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: bad chunk bounds");
  c.passes.resize(K);
  size_t w_total = 0;
  for (size_t j = 0; j < K; j++) {
    MsmCall::Pass& q = c.passes[j];
    q.lo = ranges ? (*ranges)[j].first : 0;
    q.m = ranges ? (*ranges)[j].second : n;
    if (q.m == 0 || q.lo > n || q.m > n - q.lo) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: bad chunk bounds");
    w_total += q.m;
    if (!part_make_shape(q.m, c.s.W, c.nb, &q.ps, t.part_shift))
      MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: %zu buckets / %u windows exceed the bucket sort's LDS budget (window too large)", c.nb, c.s.W);
    q.pairs = q.m * (size_t)c.s.W;
    q.max_chunks = part_max_chunks(q.pairs, q.ps.nbins);
    // [cell table: (position in the bin, start | length in the tile) per bin and tile | bin totals | bin descriptors | bucket-major segment
    //  words | tile starts (u16)]
    q.cm_bytes = (size_t)q.ps.nbins * q.ps.ntiles * sizeof(uint2);
    q.bt_bytes = ((size_t)q.ps.nbins * 4 + 15) & ~(size_t)15;
    q.bm_bytes = (size_t)q.ps.nbins * sizeof(BinMeta);
    q.sg_bytes = c.nb * sizeof(v4u_t);
    q.ts_bytes = (size_t)q.ps.ntiles * (q.ps.nbins + 1) * 2;
    c.w_digits = std::max(c.w_digits, (size_t)q.ps.ntiles * q.ps.te * 4);
    c.w_sorted = std::max(c.w_sorted, q.pairs * 4 + 16 * IDXQ_NQ);      // + 64: the bucket kernel reads the index stream in aligned 64-byte groups (segq_fetch)
    c.w_offsets = std::max(c.w_offsets, q.max_chunks * q.ps.nf * 4);
    c.w_cursor = std::max(c.w_cursor, q.cm_bytes + q.bt_bytes + q.bm_bytes + q.sg_bytes + q.ts_bytes);
    c.w_pairs = std::max(c.w_pairs, q.pairs);
  }
  if (w_total != n) MSM_REFUSE(KEAKI_ERR_BAD_ARG, "msm: the chunks cover %zu of %zu pairs", w_total, n);
#undef MSM_REFUSE
  c.u29 = std::is_same<F, Fq>::value ? t.acc_u29 : t.acc_u29_g2;              // A/B switches for profiling
  c.lazy_state = K > 1 && c.u29 && std::is_same<F, Fq>::value;                // the G1 kernel's registers stay in Acc29 between the passes
  c.hv_cap = (u32)(c.w_pairs / HEAVY_MIN + 1); c.hv_slice_cap = (u32)(c.hv_cap + c.w_pairs / HEAVY_SLICE + 1);
  c.hv_hdr = ((2 * (size_t)c.hv_cap + c.hv_slice_cap) * 4 + 255) & ~(size_t)255;
  return KEAKI_OK;
}

// The workspaces of one call as typed pointers (msm_reserve), and one pass's five arrays in `cursor` (carve)
template <class F>
struct MsmWork {
  u32 *tiles, *sorted, *hist, *segoff, *perm, *gstart, *ghist, *hv_bucket, *hv_first, *hv_owner;
  Xyzz<F> *buckets, *partials, *hv_slices;
  Acc29* state29;                  // null unless the passes park their registers
  HeavyList* hv;
  char* cursor;
  uint2* cellmeta; u32* bin_total; BinMeta* bins; v4u_t* segtab; u16* tstart;
  void carve(const MsmCall::Pass& q) {
    char *bt = cursor + q.cm_bytes, *bm = bt + q.bt_bytes, *sg = bm + q.bm_bytes, *ts = sg + q.sg_bytes;
    cellmeta = (uint2*)cursor; bin_total = (u32*)bt; bins = (BinMeta*)bm; segtab = (v4u_t*)sg; tstart = (u16*)ts;
  }
};

template <class F>
keaki_status msm_reserve(keaki_hip_ctx* ctx, MsmCall& c, MsmWork<F>& w) {
  // every workspace is reserved BEFORE the first pass (sized for the largest one): a reserve that grows a buffer waits for the stream
  // pass-1 images | bucket-ordered index stream | per-bucket counts | chunk-major segment words of the chunks beyond SEG_INLINE
  ST_TRY(reserve(ctx, ctx->digits, c.w_digits));
  ST_TRY(reserve(ctx, ctx->sorted, c.w_sorted));
  ST_TRY(reserve(ctx, ctx->hist, c.nb * 4));
  ST_TRY(reserve(ctx, ctx->offsets, c.w_offsets));
  ST_TRY(reserve(ctx, ctx->cursor, c.w_cursor));
  ST_TRY(reserve(ctx, ctx->buckets, c.nb * sizeof(Xyzz<F>)));
  ST_TRY(reserve(ctx, ctx->partials, std::max((size_t)c.rs.W * c.chunks + (size_t)c.rs.W * 256, c.rc_points) * sizeof(Xyzz<F>)));
  ST_TRY(reserve(ctx, ctx->perm, c.nb * 4 + 2 * CNT_BINS * 4 + sizeof(HeavyList)));
  ST_TRY(reserve(ctx, ctx->heavy, c.hv_hdr + (size_t)c.hv_slice_cap * sizeof(Xyzz<F>)));
  if (c.lazy_state) {
    // 144 B per bucket on top of the canonical 128 (302 MB at 2^21 buckets): optional memory like the window tables -- when it does not fit, the
    // passes go on from the canonical bucket through the saturated kernel (slower, same result) instead of failing commit / open
    const keaki_status st29 = reserve(ctx, ctx->acc29, c.nb * sizeof(Acc29));
    if (st29 == KEAKI_ERR_OOM) { c.lazy_state = false; c.u29 = false; ctx->err.clear(); }
    else if (st29 != KEAKI_OK) return st29;
  }
  w.tiles = (u32*)ctx->digits.p; w.sorted = (u32*)ctx->sorted.p; w.hist = (u32*)ctx->hist.p; w.segoff = (u32*)ctx->offsets.p;
  w.cursor = (char*)ctx->cursor.p; w.buckets = (Xyzz<F>*)ctx->buckets.p; w.partials = (Xyzz<F>*)ctx->partials.p;
  w.state29 = c.lazy_state ? (Acc29*)ctx->acc29.p : nullptr;
  w.perm = (u32*)ctx->perm.p; w.gstart = w.perm + c.nb; w.ghist = w.gstart + CNT_BINS;
  w.hv = (HeavyList*)(w.ghist + CNT_BINS);                                 // right behind the histogram: one memset clears both
  w.hv_bucket = (u32*)ctx->heavy.p; w.hv_first = w.hv_bucket + c.hv_cap; w.hv_owner = w.hv_first + c.hv_cap;
  w.hv_slices = (Xyzz<F>*)((char*)ctx->heavy.p + c.hv_hdr);
  return KEAKI_OK;
}

// The bucket sort of pass q (scal: its scalars), then the bucket schedule in descending size
template <class F>
keaki_status msm_sort_pass(keaki_hip_ctx* ctx, const MsmCall& c, const MsmCall::Pass& q, const Fr* scal, const MsmWork<F>& w) {
  const PartShape& ps = q.ps;
  const u32 nb = (u32)c.nb;
  hipStream_t st = ctx->stream;
  MsmShape sj = c.s;
  sj.n = (u32)q.m;
  const dim3 g1(ps.ntiles < ctx->n_cu ? ps.ntiles : ctx->n_cu), b1(T1_THREADS);
#define KEAKI_TILE_SORT(WS) hipLaunchKernelGGL(k_tile_sort<WS>, g1, b1, 0, st, scal, sj, ps, w.tiles, w.tstart)
  switch (sj.W) {                       // plans with 11..16 windows (what 2^16..2^26 points choose) have their digit cuts compiled in
    case 11: KEAKI_TILE_SORT(11); break;
    case 12: KEAKI_TILE_SORT(12); break;
    case 13: KEAKI_TILE_SORT(13); break;
    case 14: KEAKI_TILE_SORT(14); break;
    case 15: KEAKI_TILE_SORT(15); break;
    case 16: KEAKI_TILE_SORT(16); break;
    default: KEAKI_TILE_SORT(0); break;
  }
#undef KEAKI_TILE_SORT
  ST_TRY(launch_check(ctx, "tile_sort"));
  hipLaunchKernelGGL(k_cell_prefix, dim3(ps.nbins), dim3(1024), 0, st, (const u16*)w.tstart, ps, w.cellmeta, w.bin_total);
  hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, st, (const u32*)w.bin_total, ps.nbins, w.bins);
#define KEAKI_CHUNK_SORT1(L, R, Q, M)                                                                                                                    \
  hipLaunchKernelGGL((k_chunk_sort<L, R, Q, M>), dim3(ps.nbins), dim3(C2_THREADS), 0, st, (const u32*)w.tiles, (const uint2*)w.cellmeta, (const BinMeta*)w.bins, \
                     sj, ps, nb, w.sorted, w.segtab, w.segoff, w.hist)
#define KEAKI_CHUNK_SORT(L, R, Q) do { if (ctx->tune.cs_masked) KEAKI_CHUNK_SORT1(L, R, Q, true); else KEAKI_CHUNK_SORT1(L, R, Q, false); } while (0)
  switch (ps.geom) {                    // lanes per cell, 16-byte pieces per lane and cell, cells per group: for cells of about 18 / 36 / 72 / 144+ entries
    case 0: KEAKI_CHUNK_SORT(8, 1, 16); break;
    case 1: KEAKI_CHUNK_SORT(16, 1, 16); break;
    case 2: KEAKI_CHUNK_SORT(16, 2, 8); break;
    default: KEAKI_CHUNK_SORT(16, 4, 4); break;
  }
#undef KEAKI_CHUNK_SORT1
#undef KEAKI_CHUNK_SORT
  ST_TRY(launch_check(ctx, "chunk_sort"));
#ifdef KEAKI_DIAG
  if (ctx->tune.diag_row_mask) hipLaunchKernelGGL(k_diag_mask_rows, dim3(4096), dim3(256), 0, st, w.sorted, (size_t)q.pairs, (u32)ctx->tune.diag_row_mask);
#endif
  HIP_TRY(ctx, hipMemsetAsync(w.ghist, 0, CNT_BINS * 4 + sizeof(HeavyList), st));
  hipLaunchKernelGGL(k_cnt_hist, dim3(cdiv(nb, 1024)), dim3(256), 0, st, (const u32*)w.hist, nb, w.ghist, w.hv, c.hv_cap, c.hv_slice_cap, w.hv_bucket,
                     w.hv_first, w.hv_owner);
  hipLaunchKernelGGL(k_cnt_offsets, dim3(1), dim3(CNT_BINS), 0, st, (const u32*)w.ghist, w.gstart);
  hipLaunchKernelGGL(k_cnt_scatter, dim3(cdiv(nb, 1024)), dim3(256), 0, st, (const u32*)w.hist, nb, w.gstart, w.perm);
  return launch_check(ctx, "cnt_sort");
}

// The bucket kernel of one pass, from the switches and the pass's place in the call. G1 in the 29-bit limbs: a whole MSM (first and last)
// runs the variant acc_nt / acc_prefetch / acc_idxq name, the passes of a chunked call always the default kernel in their own mode.
template <class F>
void msm_launch_accumulate(const Tuning& t, const MsmCall& c, const Aff<F>* pts, const SortView& view, const MsmWork<F>& w, bool first, bool last,
                           hipStream_t st) {
  const dim3 ga(cdiv(c.nb, 256)), ba(256);
  const u32 *hist = w.hist, *perm = w.perm;
  const u32 nb = (u32)c.nb;
  if (c.u29) {
    if constexpr (std::is_same<F, Fq>::value) {
#define KEAKI_ACC(NT, MODE) hipLaunchKernelGGL((k_msm_accumulate_g1_u29<NT, MODE>), ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets, w.state29)
      if (first && last) {
        if (t.acc_nt) KEAKI_ACC(1, ACC_WHOLE);
        else if (!t.acc_prefetch)
          hipLaunchKernelGGL((k_msm_accumulate_g1_u29<0, ACC_WHOLE, 0>), ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets, w.state29);
        else if (!t.acc_idxq)
          hipLaunchKernelGGL((k_msm_accumulate_g1_u29<0, ACC_WHOLE, 1>), ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets, w.state29);
        else KEAKI_ACC(0, ACC_WHOLE);
      }
      else if (first) KEAKI_ACC(0, ACC_FIRST);
      else if (!last) KEAKI_ACC(0, ACC_MIDDLE);
      else KEAKI_ACC(0, ACC_LAST);
#undef KEAKI_ACC
    } else {
      if (first) hipLaunchKernelGGL(k_msm_accumulate_g2_u29<0>, ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets);
      else hipLaunchKernelGGL(k_msm_accumulate_g2_u29<1>, ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets);
    }
  } else {
    hipLaunchKernelGGL((k_msm_accumulate<F>), ga, ba, 0, st, pts, view, hist, perm, nb, w.buckets, first ? 0u : 1u);
  }
}

// The bucket kernels of one pass over the sorted stream: pts = the points (or table rows) of the pass's first pair
template <class F>
keaki_status msm_bucket_pass(keaki_hip_ctx* ctx, const MsmCall& c, const PartShape& ps, const Aff<F>* pts, const MsmWork<F>& w, bool first, bool last) {
  hipStream_t st = ctx->stream;
  const SortView view = {w.sorted, w.bins, w.segtab, w.segoff, ps};
  msm_launch_accumulate<F>(ctx->tune, c, pts, view, w, first, last, st);
  ST_TRY(launch_check(ctx, "msm_accumulate"));
  // heavy buckets (structured scalars only; the grids exit after one load otherwise)
  const u32 hv_mode = c.lazy_state && !last ? (first ? HV_SET29 : HV_ADD29) : (first ? HV_SET : HV_ADD);
  hipLaunchKernelGGL((k_msm_heavy<F>), dim3(HEAVY_GRID), dim3(256), 0, st, pts, view, (const u32*)w.hist, (const HeavyList*)w.hv, c.hv_slice_cap,
                     (const u32*)w.hv_bucket, (const u32*)w.hv_first, (const u32*)w.hv_owner, w.hv_slices);
  hipLaunchKernelGGL((k_msm_heavy_combine<F>), dim3(HEAVY_COMBINE_GRID), dim3(64), 0, st, (const u32*)w.hist, (const HeavyList*)w.hv, c.hv_cap,
                     c.hv_slice_cap, (const u32*)w.hv_bucket, (const u32*)w.hv_first, (const Xyzz<F>*)w.hv_slices, w.buckets, hv_mode, w.state29);
  return launch_check(ctx, "msm_heavy");
}

// The reduction of the buckets to the result: by row and column sums, or by running sums -> (groups of chunks) -> window sums -> Horner
template <class F>
keaki_status msm_tail(keaki_hip_ctx* ctx, const MsmCall& c, const MsmWork<F>& w, F* out) {
  hipStream_t st = ctx->stream;
  const MsmShape& rs = c.rs;
  Xyzz<F>* partials = w.partials;
  if (c.rowcol) {
    const u32 cr = rs.c, kc = (cr + 1) / 2, NC = 1u << kc, NR = 1u << (cr - kc);
    Xyzz<F>*colp = partials, *rowp = colp + (size_t)(NR / 64) * NC, *sums = rowp + (size_t)NR * (NC / 64), *planes = sums + NC + NR;
    hipLaunchKernelGGL((k_msm_rowcol<F>), dim3(2u << (cr - 12)), dim3(256), 0, st, (const Xyzz<F>*)w.buckets, cr, colp, rowp);
    hipLaunchKernelGGL((k_msm_rowcol_sums<F>), dim3((NC + NR) / 32), dim3(256), 0, st, (const Xyzz<F>*)colp, (const Xyzz<F>*)rowp, cr, sums);
    hipLaunchKernelGGL((k_msm_rowcol_planes<F>), dim3(cr + 1), dim3(256), 0, st, (const Xyzz<F>*)sums, cr, planes);
    hipLaunchKernelGGL((k_msm_rowcol_final<F>), dim3(1), dim3(64), 0, st, (const Xyzz<F>*)planes, cr + 1, out);
  } else {
    Xyzz<F>* wsums = (Xyzz<F>*)ctx->wsums.p;
    hipLaunchKernelGGL((k_msm_reduce<F>), dim3(cdiv((size_t)rs.W * c.chunks, 64)), dim3(64), 0, st, (const Xyzz<F>*)w.buckets, rs, c.L, c.chunks, partials);
    // chunk partials -> (at most 128 per window) -> window sums
    const Xyzz<F>* fin_in = partials;
    u32 fin_chunks = c.chunks;
    if (c.chunks > 256) {
      const u32 G = cdiv(c.chunks, 128);
      const u32 chunks2 = cdiv(c.chunks, G);
      Xyzz<F>* partials2 = partials + (size_t)rs.W * c.chunks;
      hipLaunchKernelGGL((k_msm_partial_groups<F>), dim3(chunks2, rs.W), dim3(64), 0, st, (const Xyzz<F>*)partials, c.chunks, G, chunks2, partials2);
      fin_in = partials2; fin_chunks = chunks2;
    }
    hipLaunchKernelGGL((k_msm_window_finish<F>), dim3(rs.W), dim3(64), 0, st, fin_in, rs, fin_chunks, wsums, rs.W == 1 ? out : (F*)nullptr);
    if (rs.W != 1) hipLaunchKernelGGL((k_msm_final<F>), dim3(1), dim3(64), 0, st, (const Xyzz<F>*)wsums, rs.W, out);
  }
  return launch_check(ctx, "msm_reduce/final");
}

// One MSM on ctx->stream: plan -> reserve -> per pass (stage, sort, bucket kernels) -> tail.
// d_table != nullptr: precomputed path (tables built by msm_build_tables with window target c_table for N = srs_len points)
template <class F>
keaki_status msm_dev(keaki_hip_ctx* ctx, const Aff<F>* d_points, size_t srs_len, const void* d_scalars, size_t n, void* d_out_jac,
                     const Aff<F>* d_table = nullptr, int c_table = 0, const MsmPipe* pipe = nullptr) {
  if (!d_out_jac || (n && (!d_points || !d_scalars))) return fail(ctx, KEAKI_ERR_BAD_ARG, "msm: null pointer");
  MsmCall c;
  const keaki_status planned = msm_plan_call<F>(ctx->tune, n, srs_len, d_table != nullptr, c_table, pipe ? &pipe->ranges : nullptr, c);
  if (planned != KEAKI_OK) return fail(ctx, planned, "%s", c.msg);
  ST_TRY(reserve(ctx, ctx->wsums, (size_t)c.rs.W * sizeof(Xyzz<F>)));
  F* out = (F*)d_out_jac;
  hipStream_t st = ctx->stream;
  if (n == 0) {
    // an empty MSM runs no window and no bucket kernel: the instrumentation (window bits, the four timing events, of which this call would
    // record the first only) stays that of the last non-empty call, also when that call is still queued in front of this one
    hipLaunchKernelGGL((k_msm_final<F>), dim3(1), dim3(64), 0, st, (const Xyzz<F>*)ctx->wsums.p, 0u, out);
    return launch_check(ctx, "msm_final");
  }
  ctx->last_c = (int)c.s.c;
  if (ctx->timing) (void)hipEventRecord(ctx->ev[0], st);
  MsmWork<F> w;
  ST_TRY(msm_reserve(ctx, c, w));
  const Aff<F>* base = c.shared ? d_table : d_points;
  const size_t K = c.passes.size();
  for (size_t j = 0; j < K; j++) {
    const MsmCall::Pass& q = c.passes[j];
    if (pipe && pipe->stage) ST_TRY(pipe->stage(j));
    w.carve(q);
    ST_TRY(msm_sort_pass(ctx, c, q, (const Fr*)d_scalars + q.lo, w));
    if (ctx->timing && j + 1 == K) (void)hipEventRecord(ctx->ev[1], st);
    ST_TRY(msm_bucket_pass(ctx, c, q.ps, base + q.lo, w, j == 0, j + 1 == K));      // table row w of point lo + i = (table + lo)[w * stride + i]
  }
  if (ctx->timing) (void)hipEventRecord(ctx->ev[2], st);
  ST_TRY(msm_tail(ctx, c, w, out));
  if (ctx->timing) {
    (void)hipEventRecord(ctx->ev[3], st);
    ctx->timing_pending = true;
  }
  return KEAKI_OK;
}

// one-time table build for the precomputed path: G1 plans of at most TABLE_MAX_W windows have a kernel of their own
template <class F>
keaki_status msm_build_tables(keaki_hip_ctx* ctx, const Aff<F>* d_points, size_t N, int c_table, Aff<F>* d_table) {
  const MsmPlan plan = msm_make_plan(N, c_table);
  const dim3 g(cdiv(N, 64)), b(64);
  if constexpr (std::is_same<F, Fq>::value) {
    if (plan.s.W <= TABLE_MAX_W) {
      hipLaunchKernelGGL(k_msm_build_tables_g1, g, b, 0, ctx->stream, d_points, (u32)N, plan.s, d_table);
      return launch_check(ctx, "msm_build_tables");
    }
  }
  hipLaunchKernelGGL((k_msm_build_tables<F>), g, b, 0, ctx->stream, d_points, (u32)N, plan.s, d_table);
  return launch_check(ctx, "msm_build_tables");
}
// window target for the shared-bucket (precomputed) path: adds = n * W(c); bucket reduction ~ 2.8 * max_b once
inline int choose_window_shared(size_t n, int forced = 0) {
  if (forced >= 3 && forced <= 24) return forced;         // Tuning::msm_c_shared
  double best = 1e300;
  int bc = 8;
  for (int c = 8; c <= 23; c++) {
    MsmPlan p = msm_make_plan(n, c);
    if (p.max_b > ((size_t)PART_MAX_BINS << PART_MAX_FINE_SHIFT)) continue;
    double cost = (double)n * p.s.W + 2.8 * (double)p.max_b;
    if ((double)p.max_b < 131072.0) cost *= 131072.0 / (double)p.max_b;
    if (cost < best) { best = cost; bc = c; }
  }
  return bc;
}
inline u32 msm_plan_windows(size_t n, int c) { return msm_make_plan(n, c).s.W; }

// window tables of N points at the automatic (or forced) shared window: the allocation is the caller's to keep
template <class F>
keaki_status msm_precompute(keaki_hip_ctx* ctx, const void* d_points, size_t N, int* c_table_out, size_t* table_bytes_out, void** d_table_out) {
  const int c = choose_window_shared(N, ctx->tune.msm_c_shared);
  const size_t bytes = (size_t)msm_plan_windows(N, c) * N * sizeof(Aff<F>);
  void* t = nullptr;
  ST_TRY(dev_alloc(ctx, &t, bytes ? bytes : 64));
  keaki_status st = msm_build_tables<F>(ctx, (const Aff<F>*)d_points, N, c, (Aff<F>*)t);
  if (st != KEAKI_OK) { (void)hipFree(t); return st; }
  *c_table_out = c; *table_bytes_out = bytes; *d_table_out = t;
  return KEAKI_OK;
}

}  // namespace keaki_internal
