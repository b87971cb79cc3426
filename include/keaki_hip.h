/* keaki_hip.h -- C ABI of libkeaki_hip.so: the MI355X (gfx950) backend for keaki's BN254 hot path.
 *
 * keaki (the reference) has no FFI of its own; its "operator API" is the generic Rust functions
 * kzg::commit/open/verify, kem::encapsulate/decapsulate and vec::vec_encrypt/vec_decrypt. Every
 * expensive step inside them is a call into arkworks. The entry points below are what a
 * feature-gated Rust shim binds in place of those arkworks calls (INTEGRATION.md shows the shim);
 * each one cites the reference line it replaces.
 *
 * Conventions
 *  - Every function returns a keaki_status (0 = ok, < 0 = error); nothing unwinds or aborts across
 *    the boundary. keaki_hip_last_error(ctx) returns a human-readable message for the last failure.
 *  - The caller owns every buffer. *_dev entry points take DEVICE pointers (memory already resident
 *    in HBM, e.g. allocated by the caller's HIP runtime) and enqueue on the ctx stream without
 *    synchronising unless stated; the plain entry points take HOST pointers, copy in/out and
 *    synchronise.
 *  - Field elements are little-endian 64-bit limbs in Montgomery form (R = 2^256) EXACTLY as ark-ff
 *    0.4.2 holds them in `Fp.0.0`, so the shim copies limbs without conversion:
 *        Fr, Fq        u64[4]
 *        G1 affine     u64[8]   (x, y);                      identity = all-zero words
 *        G1 Jacobian   u64[12]  (x, y, z) normalised: z = R (Montgomery one), identity = (R, R, 0)
 *        G2 affine     u64[16]  (x.c0, x.c1, y.c0, y.c1);    identity = all-zero words
 *        G2 Jacobian   u64[24]  normalised likewise
 *        GT            384 bytes = ark-serialize `serialize_uncompressed` of Fq12:
 *                      c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1, each canonical 32-byte LE.
 *    (arkworks' in-memory `Affine { x, y, infinity: bool }` is repr(Rust); the shim must write x,y
 *    explicitly and map `infinity` to the all-zero encoding.)
 *  - A ctx is bound to one GPU. Multi-GPU, two ways: (a) in one process, keaki_hip_group_* below (one ctx and
 *    one host thread per GPU inside the library, partial sums through host memory); (b) one process per GPU:
 *    each rank runs msm on its contiguous chunk of (scalar, point) pairs, the 96-byte partial sums are
 *    exchanged with RCCL all-gather by the caller, and keaki_hip_g1_sum_dev adds them.
 *  - Thread-safety: a ctx serialises calls internally (one recursive mutex, held from the first staging
 *    copy of a host-pointer call to its last download, so the shared staging buffers belong to one
 *    call at a time); calls from several host threads on one ctx are safe and run one after another.
 *    Use one ctx per host thread for concurrency. An SRS handle (keaki_hip_srs_*) is device memory, not
 *    context state: every ctx on the same device may pass it to msm / kzg_open / open_fk, so N threads with a
 *    ctx each share ONE copy of the points, the window tables and the FK23 transform (the handle locks its
 *    lazily built members; a handle from another device is refused with KEAKI_ERR_BAD_ARG). Handles must not
 *    be freed while another thread still uses them.
 *  - Memory: keaki_hip_ctx_memory reports what a ctx holds. Per ctx: MSM workspaces (2.4 GB at 2^24 points),
 *    pairing slots (0.48 GB), the GT tables of encapsulate (0.2 + 0.2 GB from the first encapsulation on, 2.6 + 0.2 GB once a batch >= 2^16 ran;
 *    6 MB of line tables of the multiples of g2). A ctx creates up to three non-blocking streams (its own unless one was passed in, one for
 *    the copies of chunked host-array batches, one for the table of a new commitment). Per SRS
 *    handle (shared by every ctx of the device): points (64 B each) + window tables (W x 64 B each: 12.9 GB at
 *    2^24) + the FK23 transform (192 B per opening). All optional tables fall back when they do not fit.
 *  - Current device: every call makes its ctx's GPU the calling thread's current HIP device for the duration of the
 *    call and puts the caller's own choice back before it returns; the library never calls hipDeviceReset and
 *    creates only non-blocking streams, so it can share a thread and a GPU with PyTorch or another HIP library.
 *  - The library reads the environment only inside keaki_hip_ctx_create (initial values of the tuning switches
 *    of keaki_hip_ctx_set_option); nothing on a call path calls getenv.
 */
#ifndef KEAKI_HIP_H
#define KEAKI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t keaki_status;
enum {
  KEAKI_OK = 0,
  KEAKI_ERR_BAD_ARG = -1,      /* null pointer, n out of range, n > srs length ...            */
  KEAKI_ERR_HIP = -2,          /* a HIP runtime call failed (message has hipGetErrorString)   */
  KEAKI_ERR_OOM = -3,          /* device allocation failed                                    */
  KEAKI_ERR_NO_DEVICE = -4,    /* no gfx950 device visible                                    */
  KEAKI_ERR_TOO_LARGE = -5     /* polynomial longer than the SRS: KZGError::PolynomialTooLarge */
};
enum { KEAKI_SET_MAX = 1024 };  /* most points of a KZG set opening (keaki_hip_kzg_set_polys and the calls built on it) */
enum { KEAKI_VERIFY_SETS_K_MAX = 64 };  /* most points per item of keaki_hip_kzg_verify_sets */

typedef struct keaki_hip_ctx keaki_hip_ctx;
typedef struct keaki_hip_srs_g1 keaki_hip_srs_g1; /* device-resident [tau^i]_1, affine */
typedef struct keaki_hip_srs_g2 keaki_hip_srs_g2; /* device-resident G2 bases, affine  */

/* ---- context ------------------------------------------------------------------------------- */
/* device: HIP device ordinal. stream: the hipStream_t every call of this ctx enqueues on:
 *   KEAKI_HIP_STREAM_PRIVATE  (NULL)  the ctx creates its own NON-BLOCKING stream: unordered against the caller's streams AND against the
 *                                      legacy default stream -- order *_dev calls with keaki_hip_synchronize or events;
 *   KEAKI_HIP_STREAM_LEGACY   (= hipStreamLegacy)  the legacy default ("null") stream of the device, which a NULL handle cannot name here;
 *   any other value                    a stream the caller created (e.g. the handle of a torch.cuda.Stream): *_dev calls are then ordered
 *                                      with everything else the caller enqueues there (RCCL collectives, copies). */
#define KEAKI_HIP_STREAM_PRIVATE ((void*)0)
#define KEAKI_HIP_STREAM_LEGACY ((void*)1)
keaki_status keaki_hip_ctx_create(int32_t device, void* stream, keaki_hip_ctx** out);
void keaki_hip_ctx_destroy(keaki_hip_ctx* ctx);
const char* keaki_hip_last_error(const keaki_hip_ctx* ctx); /* ctx may be NULL: last create error */
keaki_status keaki_hip_synchronize(keaki_hip_ctx* ctx);
/* the hipStream_t every call of this ctx enqueues on (for callers that order their own work -- RCCL collectives, copies -- with it) */
void* keaki_hip_ctx_stream(const keaki_hip_ctx* ctx);
/* the HIP device ordinal the ctx is bound to (-1 for NULL): for companions that make their own HIP / RCCL calls beside it (keaki_hip_rccl.h) */
int32_t keaki_hip_ctx_device(const keaki_hip_ctx* ctx);
/* "keaki-hip <ver> (gfx950) src=msm:<hash>,pairing:<hash>,fk:<hash>": the hashes of the kernel sources the binary was built from */
const char* keaki_hip_version(void);
/* keaki_hip_last_error: the returned string is a copy private to the calling thread (valid until its next call of this function). */
/* Tuning / A-B switches of a context (profiling and tests; defaults are what ships). Initial values come from the environment variable
 * KEAKI_<NAME> at keaki_hip_ctx_create; afterwards only this call changes them. Names: "msm_c", "msm_c_shared" (window bits of the MSM without / with
 * window tables: 3 .. 19 / 3 .. 23; 0 or any value outside 3 .. 24 = automatic; 20 .. 24 / 24 name plans with more buckets than the bucket sort
 * addresses and are refused with KEAKI_ERR_BAD_ARG, in the environment ignored),
 * "reduce_l", "part_shift", "acc_u29", "acc_u29_g2", "acc_nt", "acc_prefetch", "acc_idxq" (the G1 bucket kernel reads its index stream by aligned
 * 64-byte groups through a lane-private LDS slot; 0 = one 4-byte load per entry as until round 5), "cs_masked", "fk_uniform", "fk_gtab", "fk_addsub29", "fk_radix4", "fb_occ1", "gt_wb_b" (window bits of the table of
 * e(g1, g2), 0 = automatic; a change rebuilds the table on the next use), "encap_gt" (batch size from which encap_batch takes the GT
 * fixed-base path and below which -- for a commitment that has no table yet -- it runs a pairing per item; -1 = automatic: always the GT path),
 * "encap_multi_single_min" (encap_multi / encrypt_multi: a group of at least this many items runs the single-commitment path, smaller groups the
 * fused route with a pairing per item; 0 = never the single path; default 16,384, measured -- see keaki_hip_encap_multi),
 * "pair_wide_max" (pairing batches up to this size run the twelve-lanes-per-pairing kernel; -1 = automatic (4096), 0 = never), "pair_two_waves"
 * (up to 1,024 pairings: the line side of the Miller loop on a second wave; 0 = one wave), "msm_short_tables" (an MSM over less than half of an SRS
 * with window tables: 0 = the generic path as before round 4, 1 / -1 = the tables), "vec_update_k_pass" (entries of the change list per pass of
 * keaki_hip_vec_update's proof kernel: 1 .. 8, 0 = the built-in 8; any other value is refused with KEAKI_ERR_BAD_ARG, in the environment ignored),
 * "fk_coset_group" (terms per Straus group of the FK23 coset openings' pointwise kernel: 1, 2 or 4, 0 = the built-in 4; 1 = one ladder per term, the A/B
 * form), "fk_coset_min_lanes" (that kernel splits the terms of a position over lanes while its launch has fewer lanes than this: 1 .. 2^31, 0 = the
 * built-in 131,072; other values of the two are refused with KEAKI_ERR_BAD_ARG, in the environment ignored), "verify_cosets_blocks" (workgroups of
 * keaki_hip_kzg_verify_cosets' transform kernel: 1 .. 1,024, 0 = automatic, three per compute unit; results do not depend on it; other values refused),
 * "verify_sets_blocks" (workgroups of keaki_hip_kzg_verify_sets' polynomial kernel: 1 .. 1,024, 0 = automatic, three per compute unit; results do not
 * depend on it; other values refused),
 * "coset_rows_min_lanes" (keaki_hip_kzg_coset_pairs: the row kernel splits an item's l bases over lanes while a launch has fewer lanes than this: 1 .. 2^31,
 * 0 = the built-in 131,072), "coset_rows_route" (how that call sums its rows: 1 = the handle's window table over the first l SRS points, 2 = the batched
 * MSM, 0 = by plan), "coset_rows_wb" (window bits of that table: 8, 10 or 13, 0 = by plan -- the switch of the width sweep; a table the allocator refuses
 * means route 2); results do not depend on any of the three; other values are refused with KEAKI_ERR_BAD_ARG, in the environment ignored),
 * "set_rows_wb" (keaki_hip_kzg_set_pairs: window bits of the G2 handle's table, 8, 10 or 13, 0 = by plan), "set_rows_min_lanes" (its G2 row kernel splits an
 * item's k bases over lanes while a launch has fewer lanes than this: 1 .. 2^31, 0 = the built-in 65,536), "set_each_route" (keaki_hip_kzg_verify_sets_each:
 * 1 = the fused pairing kernel, 2 = two Miller loops per item through the existing kernels, 0 = by plan, which is 2); results do not depend on any of the three; other values
 * are refused with KEAKI_ERR_BAD_ARG, in the environment ignored).
 * What the library does with HOST memory of the caller, and its off switches (round 5):
 *   "host_prefault" (default 1): while the kernels of a host-array call run, the library first-touches the caller's OUTPUT arrays (writes a zero
 *       into one byte per 4 KB page, the whole range being overwritten by the download that follows; outputs >= 1 MB only) and asks for transparent
 *       huge pages on them (madvise(MADV_HUGEPAGE)); chunked batches do this on up to three helper std::threads that live for the duration of
 *       the call. 0: no helper threads, no write into and no madvise on caller memory -- every byte that appears in an output array was put there
 *       by a device-to-host copy. Results are identical; downloads into pages that do not exist yet are slower (160 MB: 30 ms instead of 3).
 *   "pipe_chunks" (default 1): host-array batches (encap / decap / encrypt / decrypt from 2 x 65,536 items on; MSMs from "msm_pipe_min" scalars on;
 *       kzg_open from 2^21 coefficients on) run as chunk pipelines over a copy stream (kzg_open: and an auxiliary stream) of the context's own.
 *       0: upload, kernels, download, in that order, on the context's stream -- for every AUTOMATIC choice. An explicit "msm_pipe_chunks" >= 2
 *       names the chunked path itself and takes precedence: a caller who wants no other stream sets "pipe_chunks" = 0 and leaves
 *       "msm_pipe_chunks" at -1 (or sets it to 0).
 *   "msm_pipe_chunks" (-1 = automatic: 6 chunks from 2^22 scalars on, 4 from 2^21, 3 from "msm_pipe_min" = 2^20 on; 0 / 1 = one copy in front; k >= 2 = k chunks at
 *       any length), "msm_pipe_growth" (size of chunk j + 1 in percent of chunk j, default 160: a short first chunk starts the device early).
 *   A host-array call of ANY entry that FAILS (status != KEAKI_OK) returns, like a successful one, only when no copy reads or writes the
 *   caller's arrays any more and nothing of the call is left on the context's side streams (pageable and pinned arrays alike). It leaves
 *   its output arrays unspecified: any prefix may hold results, and with "host_prefault" = 1 pages may hold the zeros of the first touch.
 *   Input arrays are never written.
 * Unknown name -> KEAKI_ERR_BAD_ARG. */
keaki_status keaki_hip_ctx_set_option(keaki_hip_ctx* ctx, const char* name, int64_t value);
/* Test hook: every single device allocation of this ctx above `bytes` fails with KEAKI_ERR_OOM (0 = no limit). This is how the tests
 * exercise the optional-memory fallbacks (SRS window tables, the wide GT table); nothing in the library sets it. */
keaki_status keaki_hip_debug_set_alloc_limit(keaki_hip_ctx* ctx, size_t bytes);
/* Test hook: waits for the context's streams (as keaki_hip_ctx_trim does), then sets every byte of the full capacity of every scratch workspace of
 * the context to `byte` (its low 8 bits). Nothing is freed and no capacity changes. The cached tables of encapsulate and kzg verify (guarded by their
 * ready / valid bits) and the tables of SRS handles are left alone. also_new != 0: every device allocation this context makes from now on is filled with
 * the byte as well (a grown workspace, a table before its build); also_new = 0 switches that off. A call must return the same bytes whatever the
 * workspaces held before it: this is how the tests find a read of a word the call did not write itself. ctx NULL -> KEAKI_ERR_BAD_ARG. */
keaki_status keaki_hip_debug_poison_workspaces(keaki_hip_ctx* ctx, uint32_t byte, int32_t also_new);
/* Device memory this ctx holds right now, bytes: out4[0] = window tables + FK23 transforms + coset transforms + vec_update tables of SRS handles built through this ctx (the
 * points themselves belong to the caller's upload), [1] = grow-only workspaces, [2] = fixed-base / GT tables of encapsulate, [3] = total. */
keaki_status keaki_hip_ctx_memory(keaki_hip_ctx* ctx, size_t* out4);
/* Gives back every workspace and every fixed-base / GT table of the context (out4[1] and out4[2] drop to 0): for a long-lived process after
 * an unusually large call. Everything is rebuilt on demand; results never change. SRS handles (and their tables) are the caller's. */
keaki_status keaki_hip_ctx_trim(keaki_hip_ctx* ctx);

/* ---- SRS: replaces KZGSetup::g1_aff (src/kzg.rs:22-29, built at :63) -------------------------- */
keaki_status keaki_hip_srs_g1_upload(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, keaki_hip_srs_g1** out);
/* wraps caller-owned device memory holding n affine points (not freed by _free) */
keaki_status keaki_hip_srs_g1_wrap_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, keaki_hip_srs_g1** out);
/* non-owning view of points [offset, offset + n) of `srs` (which must outlive it): the contiguous chunk one rank owns when commit's MSM
 * (src/kzg.rs:98) is sharded by point range over several GPUs; free it with keaki_hip_srs_g1_free. keaki_hip_srs_g1_precompute on
 * the view tabulates the chunk only. */
keaki_status keaki_hip_srs_g1_slice(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, size_t offset, size_t n, keaki_hip_srs_g1** out);
size_t keaki_hip_srs_g1_len(const keaki_hip_srs_g1* srs);
/* One-time precomputation for a fixed SRS (KZG bases never change): builds the window tables
 * table[w][i] = 2^(bit offset of window w) * P_i (affine, W x n x 64 bytes of HBM; W = 12..14 for n >= 2^20) so that all
 * windows of an MSM share ONE bucket set and the per-window reduction / Horner doublings disappear. Later
 * keaki_hip_msm_g1* calls on this handle with n > len/2 use the tables; results are identical. Optional. */
keaki_status keaki_hip_srs_g1_precompute(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, size_t* table_bytes_out);
void keaki_hip_srs_g1_free(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs);
keaki_status keaki_hip_srs_g2_upload(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, keaki_hip_srs_g2** out);
keaki_status keaki_hip_srs_g2_wrap_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, keaki_hip_srs_g2** out);
/* window tables of a fixed G2 basis, as keaki_hip_srs_g1_precompute (W x n x 128 bytes): removes the per-window Horner doublings of a G2 MSM */
keaki_status keaki_hip_srs_g2_precompute(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs, size_t* table_bytes_out);
void keaki_hip_srs_g2_free(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs);

/* ---- MSM: replaces <E::G1 as VariableBaseMSM>::msm_unchecked(&setup.g1_aff, p) (src/kzg.rs:98) -
 * out = sum_{i<n} scalars[i] * srs[i]; n <= len(srs) (zip-truncation as msm_unchecked).
 * n > len(srs) -> KEAKI_ERR_TOO_LARGE (the check of src/kzg.rs:93-95 lives in the caller, this is a guard).
 * out_jac: u64[12] normalised Jacobian.
 * Host-pointer form (what kzg::commit calls, src/kzg.rs:89-101: the polynomial lives in host memory): from 2^20 scalars on the vector is
 * uploaded in growing point-range chunks on the context's copy stream while the sort and bucket kernels of the chunk before run; every
 * bucket pass goes on from the state the earlier chunks left, one reduction closes the call (2^24 scalars: 18.1 ms against 28 ms with
 * the copy in front and 16.6 ms with resident scalars). The result is the same group element whatever the cut. Pageable and pinned
 * sources both work; the call returns when out_jac holds the result and no copy reads `scalars` any more. */
keaki_status keaki_hip_msm_g1(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac);
/* device-resident scalars and output (d_out_jac: 96 bytes of device memory); asynchronous on the ctx stream */
keaki_status keaki_hip_msm_g1_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_scalars, size_t n, void* d_out_jac);
/* same over G2 (no call site in keaki; north_star asks for it; out u64[24]) */
keaki_status keaki_hip_msm_g2(keaki_hip_ctx* ctx, const keaki_hip_srs_g2* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac);
keaki_status keaki_hip_msm_g2_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g2* srs, const void* d_scalars, size_t n, void* d_out_jac);
/* out = sum of k normalised-Jacobian G1 points (combines per-GPU partial sums after the all-gather) */
keaki_status keaki_hip_g1_sum_dev(keaki_hip_ctx* ctx, const void* d_points_jac, size_t k, void* d_out_jac);
keaki_status keaki_hip_g1_sum(keaki_hip_ctx* ctx, const uint64_t* points_jac, size_t k, uint64_t* out_jac);

/* ---- FK23 batch openings: replaces kzg::open_fk (src/kzg.rs:157-203; caller src/vec.rs:40) ------------------------------
 * All d = 2^log2d opening proofs of the polynomial p (d coefficients) at the d-th roots of unity, in O(d log d) group operations
 * (three G1 FFTs + 2d scalar-mults on the GPU). The scalar-field inputs are prepared by the caller (keaki's own host-side work):
 *   hat_a[2d]     = DFT_2d(0, ..., 0, p_0, ..., p_{d-1}) * (2d)^-1        (the 1/2d of the inverse transform folded in)
 *   tw_2d[d]      = omega_2d^k,  tw_2d_inv[d] = omega_2d^-k   (k < d),    tw_d[d/2] = omega_d^k   (k < d/2; not read any more, may be NULL)
 * where omega_N is ark-poly's Radix2EvaluationDomain generator of order N. Uses srs[0..d). proofs_out_aff: d affine points.
 * The SRS-only transform hat_s = DFT_2d(reversed SRS) is computed on the first call for a given d and cached in the handle. */
keaki_status keaki_hip_open_fk(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* hat_a, const uint64_t* tw_2d,
                               const uint64_t* tw_2d_inv, const uint64_t* tw_d, uint64_t* proofs_out_aff);

/* Same, from the coefficients themselves: hat_a and all twiddle tables are derived on the device (row f-4 of the scope table), the
 * caller passes only omega_2d (the order-2d root of ark-poly's Radix2EvaluationDomain), its inverse and (2d)^-1. */
keaki_status keaki_hip_open_fk_poly(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* coeffs, const uint64_t* omega_2d,
                                    const uint64_t* omega_2d_inv, const uint64_t* inv_2d, uint64_t* proofs_out_aff);
/* Optional, setup time: tabulate hat_s = DFT_2d of the reversed SRS (src/kzg.rs:166-179) for the domain size d = 2^log2d, so that the
 * first keaki_hip_open_fk[_poly] with this d does not pay for it (it depends on the SRS only; the calls cache it on first use anyway). */
keaki_status keaki_hip_srs_g1_precompute_fk(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_2d);
/* ---- FK23 sharded over `world` = 2^k ranks (one rank = one ctx = one GPU): kzg::open_fk (src/kzg.rs:157-203) of BASELINE config 5 on N GPUs.
 * The group transforms are split so that every rank does 1/world of the butterflies and of the 2d scalar-mults. The library runs NO
 * collective: a step leaves this rank's outgoing data in d_send, the CALLER exchanges (RCCL over xGMI: all-to-all with equal splits,
 * received chunks in rank order; one all-gather at the end) and hands d_recv to the next step. Steps are asynchronous on the ctx stream
 * like every *_dev entry: order the collective behind them (same stream, or keaki_hip_synchronize) and the next step behind it.
 * Needs d >= world^2 and the whole SRS (srs[0..d)) on every rank. d_send / d_recv: device buffers of sizes4[0] bytes each.
 *   setup (once per handle; the SRS-only transform, this rank's part):
 *     step 0 -> d_send | all-to-all, sizes4[1] bytes per peer | step 1 <- d_recv
 *   open (per polynomial; coeffs: d Fr on the host, the same on every rank):
 *     step 0 (coeffs) -> d_send | all-to-all, sizes4[2] per peer | step 1: d_recv -> d_send | all-to-all, sizes4[2] per peer |
 *     step 2: d_recv -> d_send = d/world affine proofs | all-gather, sizes4[3] per rank | step 3: d_recv -> proofs_out_aff (host, d affine
 *     points in natural order, the bytes keaki_hip_open_fk_poly returns).
 * A step out of order is refused (KEAKI_ERR_BAD_ARG); open step 0 may always start over. `srs` must outlive the handle. */
typedef struct keaki_hip_fk_shard keaki_hip_fk_shard;
keaki_status keaki_hip_fk_shard_create(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t rank, uint32_t world,
                                       const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d, keaki_hip_fk_shard** out);
void keaki_hip_fk_shard_free(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk);
/* sizes4[0..4): [0] = bytes of d_send / d_recv; [1] = bytes per peer of the setup's all-to-all, [2] of each of a call's two; [3] = bytes per rank of the all-gather */
keaki_status keaki_hip_fk_shard_sizes(const keaki_hip_fk_shard* fk, size_t* sizes4);
keaki_status keaki_hip_fk_shard_setup(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk, int32_t step, void* d_send, void* d_recv);
keaki_status keaki_hip_fk_shard_open(keaki_hip_ctx* ctx, keaki_hip_fk_shard* fk, int32_t step, const uint64_t* coeffs, void* d_send, void* d_recv,
                                     uint64_t* proofs_out_aff);
/* Scalar-field DFT on the device: replaces ark-poly `domain.fft` / `domain.ifft` over Fr (src/vec.rs:36-37, src/kzg.rs:185).
 * data: n = 2^log2n Fr, transformed in place: out[j] = sum_i in[i] omega^(ij), then multiplied by *scale_or_null if given
 * (pass omega^-1 and n^-1 for the inverse transform). */
keaki_status keaki_hip_fr_fft(keaki_hip_ctx* ctx, uint64_t* data, uint32_t log2n, const uint64_t* omega, const uint64_t* scale_or_null);

/* ---- vec_commit in one call: the body of vec::vec_commit (reference src/vec.rs:36-46) behind its padding draw -----------------------------
 * values: n Fr (the vector), pad: the one random scalar the caller drew (src/vec.rs:31-33; NULL: none), together the first n + 1 evaluations
 * over the domain of size d = 2^log2d (the rest are zero, as ark-poly's ifft pads). On the device, without the coefficients ever returning to
 * the host: domain.ifft (omega_d_inv = the domain's group_gen_inv, inv_d = its size_inv), the FK23 openings (omega_2d ... as for
 * keaki_hip_open_fk_poly) and the commitment (MSM over all d coefficients: trailing zeros, which DensePolynomial trims, contribute nothing).
 * com_out_jac: u64[12] normalised Jacobian; proofs_out_aff: d affine points. Needs d <= len(srs). */
keaki_status keaki_hip_vec_commit(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const uint64_t* values, size_t n, const uint64_t* pad, uint32_t log2d,
                                  const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d, const uint64_t* omega_2d_inv,
                                  const uint64_t* inv_2d, uint64_t* com_out_jac, uint64_t* proofs_out_aff);

/* ---- vec_update: change k evaluations of a committed vector, the commitment and all d proofs follow ---------------------------------------------
 * The holder of (com, proofs) of keaki_hip_vec_commit changes evaluation idx[t] by deltas[t] (t < k) WITHOUT the vector: afterwards com and
 * proofs are byte for byte what keaki_hip_vec_commit returns for the changed vector (proofs are affine, the commitment a normalised Jacobian:
 * both forms are unique). With w = omega_d, c_i = w^i / d and two tables of d G1 points that depend on (srs, d) only,
 *   a_i = w^-i sum_k w^(-ik) srs[k] = [(tau^d - 1) / (tau - w^i)]_1,   u_i = (w^-i / d) sum_k (d-1-k) w^(-ik) srs[k] = [(L_i(tau) - 1) / (tau - w^i)]_1,
 *   com'  = com  + sum_t (delta_t c_(i_t)) a_(i_t)
 *   pi_j' = pi_j + sum_{t: i_t != j} s_tj (a_(i_t) - a_j) + sum_{t: i_t = j} delta_t u_j,   s_tj = delta_t c_(i_t) / (w^(i_t) - w^j)
 * (identities in tau: any SRS, tau = 0 and tau on the domain included): (k + 1) d scalar multiples instead of the d (log2 d + 3) of FK23.
 *   indices    address the evaluations over the whole domain (the padding slot of vec_commit is an ordinary index); duplicates add; delta = 0
 *              is an ordinary entry. k = 0, or both outputs NULL, writes nothing and returns KEAKI_OK. Either output may be NULL.
 *   routes     the list runs in passes of 8 entries (option "vec_update_k_pass": 1 .. 8, 0 = 8): one kernel per pass, one lane per proof,
 *              every pass a complete update of its own entries. The commitment is k scalar multiples and a sum.
 *   tables     192 B x d (a, u, w^-i, 1 / (w^t - 1)), built on first use or by keaki_hip_srs_g1_precompute_update, cached in the SRS handle for ONE d
 *              (another d replaces them) beside the FK23 transform, which they never evict; built under the handle's lock, counted in
 *              keaki_hip_ctx_memory out4[0], freed with the handle.
 *   errors     a null required pointer, an index >= d, log2d > 27, k >= 2^31 -> KEAKI_ERR_BAD_ARG; d > len(srs) -> KEAKI_ERR_TOO_LARGE; tables (or
 *              workspace) the device or keaki_hip_debug_set_alloc_limit refuses -> KEAKI_ERR_OOM. Nothing is written in any of these cases and
 *              the context stays usable.
 *   host form  one upload (indices, deltas, com, proofs), the kernels, one download; returns only when nothing reads or writes caller memory.
 *   _dev       idx (u32), deltas, com, proofs are device pointers (16-byte aligned; idx 4-byte), the domain constants stay host pointers;
 *              asynchronous on the ctx stream. The indices cannot be checked without a round trip: an entry with an index >= d does nothing.
 *   numbers    (MI355X, medians, one process, alternating rounds: profiles/vec_update_times.txt, bench_tools/bench_vec_update.py) against
 *              keaki_hip_vec_commit at the same d on a handle with window tables, resident / from host arrays:
 *                d = 2^12: commit 19 ms;  update k = 1: 3.1 / 3.2 ms, k = 4: 4.2 / 4.3, k = 16: 10 / 10, k = 64: 38 / 38, k = 256: 147 / 147
 *                d = 2^16: commit 31 ms;  update k = 1: 3.3 / 3.5 ms, k = 4: 4.4 / 4.6, k = 16: 11 / 11, k = 64: 39 / 39, k = 256: 150 / 150
 *                d = 2^20: commit 238 ms (207 resident);  update k = 1: 23 / 26 ms, k = 4: 36 / 39, k = 16: 102 / 105, k = 64: 401 / 405, k = 256: 1,598 / 1,601
 *              so one changed entry costs a ninth of a fresh commitment at 2^16 and 2^20 (a sixth at 2^12). A pass of 8 entries costs about 5 ms up
 *              to d = 2^16 (one chain per lane: latency) and 50 ms at 2^20. Crossover, where the update stops winning and the caller should call
 *              keaki_hip_vec_commit instead: k = 16 still wins and k = 64 loses at every measured d; by the pass cost the break-even lies near
 *              k = 32 at 2^12 and 2^20 and near k = 48 at 2^16 (not measured between 16 and 64). Table build: 35 / 30 / 198 ms, 0.75 / 12 / 192 MB. */
keaki_status keaki_hip_srs_g1_precompute_update(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                                const uint64_t* inv_d);     /* setup-time, optional: vec_update builds the tables on first use anyway */
keaki_status keaki_hip_vec_update(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                  const uint64_t* inv_d, const uint32_t* idx, const uint64_t* deltas, size_t k, uint64_t* com_inout_jac,
                                  uint64_t* proofs_inout_aff);
keaki_status keaki_hip_vec_update_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* omega_d, const uint64_t* omega_d_inv,
                                      const uint64_t* inv_d, const void* d_idx, const void* d_deltas, size_t k, void* d_com_inout_jac,
                                      void* d_proofs_inout_aff);

/* ---- KZG `open` in one call (scope row f-4) -------------------------------------------------------------------------
 * Replaces the body of `open` (reference src/kzg.rs:104-124): value = p(point) and proof = commit(q), q = (p - p(point)) / (x - point),
 * with the synthetic division done on the device (blockwise Horner recurrence) right in front of the MSM, so the n - 1 quotient
 * coefficients never exist on the host. coeffs: n Fr, low degree first, trailing zeros already trimmed as ark-poly's
 * DensePolynomial does. n - 1 must not exceed the SRS length (KEAKI_ERR_TOO_LARGE; the caller raises PolynomialTooLarge first,
 * src/kzg.rs:113-118). proof_out_jac: u64[12] normalised Jacobian; value_out: u64[4] or NULL. */
keaki_status keaki_hip_kzg_open(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* point,
                                uint64_t* proof_out_jac, uint64_t* value_out);

/* The quotient alone, for callers that run the MSM elsewhere (keaki_hip_group_kzg_open does): quotient_out = n - 1 Fr (may be NULL when
 * n <= 1), value_out = p(point) (u64[4] or NULL). Same recurrence as keaki_hip_kzg_open, host pointers in and out. */
keaki_status keaki_hip_kzg_quotient(keaki_hip_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* point, uint64_t* quotient_out,
                                    uint64_t* value_out);

/* ---- KZG set openings: ONE proof for k points ----------------------------------------------------------------------------------------------
 * Beyond the reference (whose open / verify, src/kzg.rs:104-148, take one point): the batch opening of the original KZG paper. For the set
 * S = {z_0 .. z_(k-1)} of DISTINCT points, Z(x) = prod (x - z_j), I = the interpolant of (z_j, y_j) (deg < k) and the weights
 * c_j = 1 / Z'(z_j) = 1 / prod_(t != j) (z_j - z_t):
 *     pi_S = [((p - I) / Z)(tau)]_1 = sum_j c_j pi_j           e(C - [I(tau)]_1, g2) == e(pi_S, [Z(tau)]_2)
 * (pi_j the single openings: partial fractions of 1 / Z). One 64-byte proof and two pairings whatever k is.
 *   distinct   The library does NOT look for repeated points: a repeated z_j makes a weight 0 and every result meaningless. Distinct points
 *              are the caller's contract; the host layers (host/keaki.cpp, rust/keaki/src/hip.rs) sort a copy and refuse a repeat.
 *   layout     points, values, weights: k Fr; z_coeffs_out: k + 1 Fr, low degree first (monic); i_coeffs_out: k Fr, low degree first; proofs_aff:
 *              k x u64[8] affine; proof_out_jac: u64[12] normalised Jacobian (a unique form: equal group elements give equal bytes).
 *   set_polys  Z, the weights and, when values is given, I (values NULL: i_coeffs_out must be NULL): one workgroup, O(k^2) Fr products.
 *   open_multi proof and values_out[j] = p(z_j) (values_out may be NULL) from the n coefficients: the quotient (p - I) / Z is computed on the device
 *              as sum_j c_j (p - p(z_j)) / (x - z_j), the blockwise recurrence of keaki_hip_kzg_open for 8 points side by side (every coefficient is
 *              read once per pass of 8 points: ceil(k / 8) passes), in front of ONE MSM over n - 1 terms (the top k - 1 are zero in Fr), which
 *              uses the handle's window tables exactly as keaki_hip_kzg_open does. k = 1 is byte for byte keaki_hip_kzg_open. n <= k: the proof
 *              is the identity (R, R, 0), the values are still written; n = 0: zero values.
 *   aggregate  pi_S = sum_j c_j pi_j from the k single proofs, without the polynomial: the weights, then one MSM over the proofs as an ad-hoc
 *              base vector. Byte for byte open_multi's proof for the same set.
 *   verify_multi  [Z(tau)]_2 by an MSM over the first k + 1 points of srs_g2 ([tau^i]_2), [I(tau)]_1 by an MSM over the first k points of srs_g1,
 *              then the predicate through keaki_hip_kzg_verify itself with com := C - [I]_1, value := 0, point := 0, tau_g2 := [Z]_2.
 *              *ok_out = 1 / 0. pair_out_aff (or NULL): C - [I]_1 (u64[8]) then [Z]_2 (u64[16]), affine. Host arrays only.
 *   errors     k = 0 or k > KEAKI_SET_MAX, a null required pointer, i_coeffs_out without values -> KEAKI_ERR_BAD_ARG; n - 1 > len(srs), k + 1 >
 *              len(srs_g2), k > len(srs_g1) -> KEAKI_ERR_TOO_LARGE; a refused workspace -> KEAKI_ERR_OOM. Nothing is written in any of these cases
 *              and the context stays usable.
 *   host form  one upload in front of the kernels (open_multi does NOT run the chunk pipeline of keaki_hip_kzg_open: the coefficients are
 *              uploaded whole, whatever n is), the kernels, one download; returns only when nothing reads or writes caller memory.
 *   _dev       every array is a device pointer (16-byte aligned); asynchronous on the ctx stream. Workspace grow-only, counted in
 *              keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim.
 *   numbers    (MI355X, medians, one process, alternating rounds, resident: profiles/open_multi_times.txt, bench_tools/bench_open_multi.py) open_multi at
 *              k = 2 / 8 / 64: 2^24 coefficients 18.3 / 24.5 / 80.6 ms (one MSM of that size 15.8; k calls of keaki_hip_kzg_open from host arrays 41 / 159 /
 *              1,224), 2^20: 3.0 / 4.9 / 23 ms (8.5 / 26 / 188), 2^12: 1.6 / 2.8 / 14 ms -- where k = 64 LOSES to keaki_hip_kzg_open_batch_dev + aggregate
 *              (7.0 ms): short polynomials with many points belong there. The fused quotient beats k single-point quotients at every size measured
 *              (2^24, k = 64: 65 against 105 ms). verify_multi: 8 - 9 ms whatever k is (k single verifications: 3.4 ms at k = 2, 13.4 at 8, 108 at 64). */
keaki_status keaki_hip_kzg_set_polys(keaki_hip_ctx* ctx, const uint64_t* points, const uint64_t* values, size_t k, uint64_t* z_coeffs_out,
                                     uint64_t* weights_out, uint64_t* i_coeffs_out);
keaki_status keaki_hip_kzg_set_polys_dev(keaki_hip_ctx* ctx, const void* d_points, const void* d_values, size_t k, void* d_z_coeffs_out,
                                         void* d_weights_out, void* d_i_coeffs_out);
keaki_status keaki_hip_kzg_open_multi(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* points, size_t k,
                                      uint64_t* proof_out_jac, uint64_t* values_out);
keaki_status keaki_hip_kzg_open_multi_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, const void* d_points, size_t k,
                                          void* d_proof_out_jac, void* d_values_out);
keaki_status keaki_hip_kzg_aggregate(keaki_hip_ctx* ctx, const uint64_t* points, const uint64_t* proofs_aff, size_t k, uint64_t* proof_out_jac);
keaki_status keaki_hip_kzg_aggregate_dev(keaki_hip_ctx* ctx, const void* d_points, const void* d_proofs_aff, size_t k, void* d_proof_out_jac);
keaki_status keaki_hip_kzg_verify_multi(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                        const uint64_t* points, const uint64_t* values, size_t k, const uint64_t* proof_aff, int32_t* ok_out,
                                        uint64_t* pair_out_aff);

/* ---- FK23 coset openings: all d / l set proofs of a vector in one call (FK20 / FK23 "multi-reveal") ------------------------------------------
 * The set-opening counterpart of keaki_hip_open_fk_poly. p has d = 2^log2d coefficients, l = 2^log2l <= d, r = d / l. Coset i < r is the index set
 * {i + t r : t < l} of the size-d evaluation domain: the l solutions of x^l = c_i, c_i = omega_r^i. Its proof is pi_i = [floor(p / (x^l - c_i))(tau)]_1,
 * which is what keaki_hip_kzg_open_multi returns for those l points. All r proofs come out of one pass: the 2d scalar multiples that FK23 pays,
 * summed l at a time into 2r points, then group transforms of size 2r and r instead of 2d and d (derivation: csrc/fk_coset.hip).
 *   arguments  omega_2r: the generator of ark-poly's Radix2EvaluationDomain of size 2r (= omega_2d^l), omega_2r_inv its inverse, inv_2r = (2r)^-1; the
 *              library derives omega_r and every twiddle on the device. coeffs: d Fr (a shorter polynomial is zero-padded by the caller). hat_a (the
 *              raw form, for tests that choose the scalars): l rows of 2r Fr, row j at hat_a + 4 * 2r * j words in natural order, row j =
 *              DFT_2r(r zeros, then f_(u l + j), u < r) with the (2r)^-1 folded in -- as keaki_hip_open_fk takes its hat_a.
 *   results    proofs_out_aff: r affine points in natural order, (0, 0) for the identity; proof i belongs to c_i = omega_r^i and is byte for byte the
 *              affine form of keaki_hip_kzg_open_multi on coset i. log2l = 0: the bytes of keaki_hip_open_fk_poly. r = 1: one identity, no transform runs.
 *   errors     a null required pointer, log2l > log2d, log2d > 27, l > KEAKI_SET_MAX (so every proof can be checked by keaki_hip_kzg_verify_multi) ->
 *              KEAKI_ERR_BAD_ARG; d > len(srs) -> KEAKI_ERR_TOO_LARGE; a refused cache or workspace -> KEAKI_ERR_OOM. Nothing is written in any of
 *              these cases and the context stays usable.
 *   cache      the l transforms of the SRS rows depend on (srs, d, l) only: 2d JACOBIAN points (192 B x d; the form the group transform leaves, the
 *              ladder's table build reads any Z), built on first use or by keaki_hip_srs_g1_precompute_fk_cosets, cached in the SRS handle for ONE
 *              (log2d, log2l) beside -- and never evicting -- the FK23 transform and the vec_update tables; another pair replaces them. Counted in
 *              keaki_hip_ctx_memory out4[0], freed with the handle.
 *   kernel     one lane per position q < 2r (or per slice of its l terms: below "fk_coset_min_lanes" lanes -- default 131,072: two resident waves per SIMD,
 *              set from the threshold sweep of profiles/fk_coset_times.txt -- the terms of a position are split over S lanes and the partial sums added). A lane runs its terms in groups of G = 4 (option
 *              "fk_coset_group": 1, 2, 4): GLV halves in signed 4-bit windows, G window tables of 1 KB in a lane-contiguous workspace on ONE working
 *              curve, ONE chain of 129 doublings per group with 66 G mixed additions.
 *   host form  one upload, the kernels, one download; returns only when nothing reads or writes caller memory.
 *   _dev       d_coeffs and d_proofs_out_aff are device pointers (16-byte aligned), the domain constants stay host pointers (read before the call
 *              returns); asynchronous on the ctx stream. Workspace grow-only, counted in keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim.
 *   numbers    (MI355X, medians, one process, alternating rounds, cache warm: profiles/fk_coset_times.txt, bench_tools/bench_fk_coset.py) resident, l = 4 / 16 /
 *              64: d = 2^20 82 / 48 / 42 ms against 200 for keaki_hip_open_fk_poly at the same d; 2^16 26 / 21 / 16 against 30; 2^12 16 / 12 / 10
 *              against 67 (19 from host arrays); host arrays cost at most 1 ms more. The parent's routes for the same r proofs, extrapolated from 64
 *              cosets: open_fk_poly + r aggregations 37 s and r open_multi calls 371 s at d = 2^20, l = 64. Cache build 32 - 835 ms (one transform per
 *              row). At d = 2^20 the pointwise kernel takes 15 / 17 / 18 ms with G = 4 and 21 / 24 / 24 with one ladder per term; at d <= 2^16 its launch
 *              is too small to fill the device and G = 1 is the faster form (1.5 against 2.1 ms of 16 - 26): the tail of small transforms dominates there. */
keaki_status keaki_hip_srs_g1_precompute_fk_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* omega_2r);
keaki_status keaki_hip_open_fk_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* hat_a, const uint64_t* omega_2r,
                                      const uint64_t* omega_2r_inv, uint64_t* proofs_out_aff);
keaki_status keaki_hip_open_fk_cosets_poly(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const uint64_t* coeffs,
                                           const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const uint64_t* inv_2r, uint64_t* proofs_out_aff);
keaki_status keaki_hip_open_fk_cosets_poly_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, uint32_t log2l, const void* d_coeffs,
                                               const uint64_t* omega_2r, const uint64_t* omega_2r_inv, const uint64_t* inv_2r, void* d_proofs_out_aff);

/* ---- batched commit and open: m polynomials over ONE SRS in one call ---------------------------------------------------------------------
 * Generalises `commit` (reference src/kzg.rs:89-101) and `open` (src/kzg.rs:104-124) from one polynomial to m rows. A single MSM costs
 * 0.4 .. 2.3 ms of launch latency whatever its length; m short rows in one call pay that floor once.
 *   layout     row j is n Fr at scalars + 4 * stride * j (64-bit words), stride >= n in Fr units; the gap between rows is never read.
 *              out_jac / proofs_out_jac: m x u64[12] normalised Jacobian; points: m Fr (z_j); values_out: m Fr or NULL.
 *   lengths    rows of unequal length are padded with zero coefficients up to n: a zero scalar contributes nothing to the sum, which is what
 *              the trimming of ark-poly's DensePolynomial means. For open_batch every row has length n after padding, the quotient n - 1
 *              terms; the trailing zero terms of a shorter row's quotient are harmless, value and proof are those of the trimmed polynomial.
 *   results    out[j] is byte for byte what keaki_hip_msm_g1 returns for row j alone, (proofs[j], values[j]) what keaki_hip_kzg_open returns
 *              for (row j, points[j]) -- on a handle with window tables and on one without, and whichever route the call takes: rows of up to
 *              16,384 coefficients (N_BATCH_MAX) run the batch kernels, which read the SRS points only; longer rows, and calls whose
 *              workspace the device (or keaki_hip_debug_set_alloc_limit) refuses, run the single-MSM pipeline row by row.
 *   errors     n > len(srs) (open_batch: n - 1 > len(srs)) -> KEAKI_ERR_TOO_LARGE (the caller raises PolynomialTooLarge first, src/kzg.rs:93-95,
 *              :113-118). A null pointer, stride < n, m * n >= 2^31 -> KEAKI_ERR_BAD_ARG. m = 0 writes nothing and returns KEAKI_OK (only srs,
 *              stride and the product are looked at). n = 0 writes m identities (R, R, 0), open_batch also m zero values.
 *   host form  one upload of the rows in front (the span from row 0 to the end of row m - 1), the kernels, one download of m x 96 B (open_batch:
 *              + m x 32 B): no chunk pipeline, the copy stream and the helper threads of the long single calls are not used.
 *   _dev       every array is a device pointer (16-byte aligned); asynchronous on the ctx stream like keaki_hip_msm_g1_dev.
 *   context    the ctx lock is held for the call and the caller's current device is put back. Workspace: 32 B per scalar of a pass (at most
 *              256 MB unless one row is longer) + 128 B per row and window (open_batch: + the quotient rows), grow-only, counted in
 *              keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim.
 *   After a batch call the values of keaki_hip_last_msm_bucket_ms / _total_ms / _window_bits are unspecified. */
keaki_status keaki_hip_msm_g1_batch(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* scalars, size_t n, size_t m, size_t stride,
                                    uint64_t* out_jac);          /* m x commit's MSM, src/kzg.rs:89-101 (:98) */
keaki_status keaki_hip_msm_g1_batch_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_scalars, size_t n, size_t m, size_t stride,
                                        void* d_out_jac);        /* src/kzg.rs:89-101, device-resident rows */
keaki_status keaki_hip_kzg_open_batch(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const uint64_t* coeffs, size_t n, size_t m, size_t stride,
                                      const uint64_t* points, uint64_t* proofs_out_jac, uint64_t* values_out);    /* m x open, src/kzg.rs:104-124 */
keaki_status keaki_hip_kzg_open_batch_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, const void* d_coeffs, size_t n, size_t m, size_t stride,
                                          const void* d_points, void* d_proofs_out_jac, void* d_values_out);      /* src/kzg.rs:104-124, device-resident */

/* ---- batched FK23 openings and vec_commit: m small vectors over ONE domain in one call ------------------------------------------------------
 * keaki_hip_open_fk_poly and keaki_hip_vec_commit are built for one large domain; at d = 2^8 a call is ~67 launches of 128 lanes. Here m rows
 * pay every launch once, and because the rows of a pass share the twiddle of every butterfly, all stages run the shared-scalar ladder.
 *   layout     as keaki_hip_msm_g1_batch: row j at base + 4 * stride * j (64-bit words), stride in Fr units; the gap between rows is never read.
 *              open_fk_poly_batch: a row is d = 2^log2d coefficients, stride >= d. vec_commit_batch: a row is its first n <= d evaluations,
 *              stride >= n, with the padding scalar of src/vec.rs:31-33 already appended by the caller (row j = vec_j | r_j | 0...: vectors of
 *              unequal length share one call); evaluations n .. d - 1 are zero, as ark-poly's ifft resizes. There is no `pad` argument.
 *              proofs_out_aff: m x d affine points, row j's proofs in natural order at proofs + 8 * d * j; com_out_jac: m x u64[12] normalised Jacobian.
 *   results    row j is byte for byte what keaki_hip_open_fk_poly returns for that row alone, and what keaki_hip_vec_commit returns for it with
 *              values = the row and pad = NULL -- whichever route the call takes, on a handle with window tables and on one without.
 *   routes     d = 2 .. 4,096 (FKB_LOG2D_MAX = 12) run the batch kernels in passes of whole rows: at most 256 MB of workspace (288 d bytes per
 *              row, rows in groups of 64) and 16,384 rows a pass; a workspace the device (or keaki_hip_debug_set_alloc_limit) refuses halves the
 *              pass. Larger domains, d = 1, and calls refused down to a single row run the single pipeline row by row, unchanged. The m
 *              commitments are keaki_hip_msm_g1_batch_dev over the coefficient rows, with its own routes.
 *   errors     a null pointer, stride too small, n > d, m * d >= 2^31, log2d > 27 -> KEAKI_ERR_BAD_ARG; d > len(srs) -> KEAKI_ERR_TOO_LARGE, as
 *              the single calls. m = 0 writes nothing and returns KEAKI_OK.
 *   host form  one upload of the rows (the span from row 0 to the end of row m - 1), the kernels, one download; no chunk pipeline. A failing
 *              call returns only when nothing reads or writes caller memory any more.
 *   _dev       every array is a device pointer (16-byte aligned); the three to five domain constants stay host pointers (read before the call
 *              returns); asynchronous on the ctx stream like keaki_hip_msm_g1_batch_dev.
 *   context    the ctx lock and the handle's lock are held for the call; the handle's cached transform is used and, at another d, replaced
 *              exactly as by a single call. Workspace grow-only, counted in keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim. */
keaki_status keaki_hip_open_fk_poly_batch(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const uint64_t* coeffs, size_t m, size_t stride,
                                          const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d,
                                          uint64_t* proofs_out_aff);     /* m x kzg::open_fk, src/kzg.rs:157-203 */
keaki_status keaki_hip_open_fk_poly_batch_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2d, const void* d_coeffs, size_t m, size_t stride,
                                              const uint64_t* omega_2d, const uint64_t* omega_2d_inv, const uint64_t* inv_2d, void* d_proofs_out_aff);
keaki_status keaki_hip_vec_commit_batch(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const uint64_t* evals, size_t n, size_t m, size_t stride,
                                        uint32_t log2d, const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d,
                                        const uint64_t* omega_2d_inv, const uint64_t* inv_2d, uint64_t* com_out_jac,
                                        uint64_t* proofs_out_aff);       /* m x the body of vec::vec_commit, src/vec.rs:36-46 */
keaki_status keaki_hip_vec_commit_batch_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, const void* d_evals, size_t n, size_t m, size_t stride,
                                            uint32_t log2d, const uint64_t* omega_d_inv, const uint64_t* inv_d, const uint64_t* omega_2d,
                                            const uint64_t* omega_2d_inv, const uint64_t* inv_2d, void* d_com_out_jac, void* d_proofs_out_aff);

/* ---- KZG `verify` in one call -------------------------------------------------------------------------------------
 * Replaces the body of `verify` (reference src/kzg.rs:127-146): e(com - value g1, g2) == e(proof, [tau]_2 - point g2).
 * Evaluated exactly in that form: the two inner points are fixed-base sums over 8-bit window tables of g1 and g2 (built at the first
 * call of a context), the two pairings one launch of the low-latency pairing kernel. (Until round 4: e(com - value g1 + point proof, g2)
 * == e(proof, [tau]_2) -- the same predicate by bilinearity, tabulated lines, but a variable-base ladder in front.)
 * com_aff, proof_aff: u64[8] affine G1 ((0,0) = identity);
 * tau_g2_aff: u64[16]; point, value: u64[4] Fr. *ok_out = 1 when the equation holds, else 0. */
keaki_status keaki_hip_kzg_verify(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* point,
                                  const uint64_t* value, const uint64_t* proof_aff, int32_t* ok_out);

/* ---- KZG batch verification: n openings in one call ------------------------------------------------------------------
 * Generalises `verify` (reference src/kzg.rs:127-148) to n openings (C_i, z_i, y_i, proof_i) by a linear combination with the caller's
 * coefficients gamma_i:
 *     L = sum gamma_i C_i - (sum gamma_i y_i) g1 + sum (gamma_i z_i) proof_i        R = sum gamma_i proof_i
 *     *ok_out = 1  <=>  e(L, g2) == e(R, [tau]_2)
 * which is sum gamma_i x (the predicate of src/kzg.rs:135-148 with z_i proof_i moved across the pairing). Cost: one pass over the scalars, two
 * MSMs over the proofs (three with com_stride = 1), two pairings in one launch -- not 2n pairings.
 * The call evaluates EXACTLY this equation for the gammas it is given; that is a deterministic contract. If all n openings are valid it
 * always accepts. If one is invalid it rejects except with probability <= 1/r -- PROVIDED the gamma_i are independent, uniform in Fr and
 * unknown to whoever produced the proofs. Badly chosen gammas void the bound: with all gamma_i equal, two errors can cancel (y_0 + d and
 * y_1 - d are accepted together), and gamma = 0 accepts anything. gammas are drawn by the caller, one Fr::rand per item in index order (the
 * rule encap_batch follows for r), so the randomness stream stays the caller's and every result is reproducible.
 *   com_aff      com_stride = 0: ONE affine G1 point u64[8], the commitment of all items; 1: n points, com_aff[i] belongs to item i
 *   tau_g2_aff   u64[16]
 *   points       point_mode = 0: n Fr, z_i; 1: ONE Fr omega, item i is opened at omega^i (the powers are derived on the device)
 *   values, gammas   n Fr each;   proofs_aff   n affine G1 points
 *   sums_out_aff u64[16] = L then R, affine ((0,0) = identity), or NULL: what the two pairings were evaluated on
 * Identity commitments and proofs, zero values / points / gammas are ordinary inputs (L = R = identity is accepted: both sides are GT one).
 * n = 0: *ok_out = 1, the sums are the identity. com_stride or point_mode outside {0, 1}, a null pointer: KEAKI_ERR_BAD_ARG.
 * Host form: from 65,536 items on the arrays (160 B per item) go up on the context's copy stream in the order the kernels read them (gammas and
 * proofs first); the call returns when the results are in place and no copy reads caller memory any more, also on failure.
 * _dev: every array is a device pointer (the commitment, [tau]_2 and omega too); ok_out and sums_out_aff stay HOST pointers, so this form
 * synchronises as well. Workspace: 32 B per item + 67 KB, grow-only, besides the MSM's own. */
keaki_status keaki_hip_kzg_verify_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, int32_t com_stride, const uint64_t* tau_g2_aff,
                                        const uint64_t* points, int32_t point_mode, const uint64_t* values, const uint64_t* proofs_aff,
                                        const uint64_t* gammas, size_t n, int32_t* ok_out, uint64_t* sums_out_aff);
keaki_status keaki_hip_kzg_verify_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, int32_t com_stride, const void* d_tau_g2_aff,
                                            const void* d_points, int32_t point_mode, const void* d_values, const void* d_proofs_aff,
                                            const void* d_gammas, size_t n, int32_t* ok_out, uint64_t* sums_out_aff);

/* ---- KZG coset batch verification: n set proofs over cosets of one size in one call ----------------------------------------------------------
 * The verifier's counterpart of keaki_hip_open_fk_cosets: what keaki_hip_kzg_verify_multi checks one proof at a time, for n items at once. l =
 * 2^log2l, omega_l the generator of ark-poly's Radix2EvaluationDomain of size l. Item k < n: a commitment C_k, a shift h_k != 0, the l claimed
 * values y_(k,t) = p_k(h_k omega_l^t), a proof pi_k, the caller's coefficient gamma_k. Every coset of size l has Z(X) = X^l - c, c_k = h_k^l, so all
 * items share ONE G2 point [tau^l]_2 and the per-item part of Z crosses the pairing as a G1 scalar. The single check (verify_multi's on those l points):
 *     e(C_k - [I_k(tau)]_1, g2) == e(pi_k, [tau^l]_2 - c_k g2)      I_k(X) = sum_j a_(k,j) X^j,   a_(k,j) = h_k^-j l^-1 sum_t y_(k,t) omega_l^(-j t)
 * The call evaluates EXACTLY this combination:
 *     J_j = sum_k gamma_k a_(k,j)  (j < l)       L = sum_k gamma_k C_k - sum_j J_j [tau^j]_1 + sum_k (gamma_k c_k) pi_k       R = sum_k gamma_k pi_k
 *     *ok_out = 1  <=>  e(L, g2) == e(R, [tau^l]_2)
 * for the gammas it is given; that is a deterministic contract. If all n items are valid it always accepts. If one is invalid it rejects except
 * with probability <= 1/r -- PROVIDED the gamma_k are independent, uniform in Fr and unknown to whoever produced the proofs. Badly chosen gammas
 * void the bound: with all gamma_k equal, two errors can cancel (y_(0,t) + d and y_(1,t) - d at equal shifts are accepted together), and gamma = 0
 * accepts anything. gammas are drawn by the caller, one Fr::rand per item in index order (the rule encap_batch follows for r), so the randomness
 * stream stays the caller's and every result is reproducible. At l = 1 the equation is keaki_hip_kzg_verify_batch's with z_k = h_k (and
 * [tau^0]_1 = g1 = the first point of srs_g1): sums_out_aff is byte for byte what that call returns.
 *   srs_g1       the handle whose first l points [tau^j]_1 the MSM with -J reads
 *   com_aff      com_stride = 0: ONE affine G1 point u64[8], the commitment of all items (a vector's cosets); 1: n points
 *   tau_l_g2_aff u64[16]: [tau^l]_2, passed by the caller as verify_batch takes [tau]_2 (point l of a G2 SRS)
 *   points       point_mode = 0: n Fr, h_k; 1: ONE Fr omega, item k has h_k = omega^k (derived on the device). Coset i of keaki_hip_open_fk_cosets is
 *                {i + t r}: h = omega_d^i, so all r cosets of a vector are point_mode 1 with omega_d.
 *   values       value (k, t) is the Fr at values + 4 (k item_stride + t t_stride) words. Rows: (item_stride, t_stride) = (l, 1). A vector of d = r l
 *                evaluations in domain order, all r cosets: (1, r) with n = r.
 *   omega_l_inv, inv_l   u64[4] each: omega_l^-1 and l^-1 (the library derives every h_k^-1 itself: one Fermat inversion per 16 items)
 *   proofs_aff, gammas   n affine G1 points, n Fr;   sums_out_aff u64[16] = L then R, affine ((0,0) = identity), or NULL
 *   zero shift   h_k = 0 is no coset. The library does NOT look: the inverses of the 16 items that share its inversion come out 0 and the results
 *                are meaningless. Non-zero shifts are the caller's contract; the host layers (host/keaki.cpp, rust/keaki/src/hip.rs) refuse a zero.
 * Identity commitments and proofs, zero values and gammas are ordinary inputs. n = 0: *ok_out = 1, the sums are the identity.
 *   errors     a null required pointer, com_stride or point_mode outside {0, 1}, l > KEAKI_SET_MAX, n l >= 2^31, strides under which two values of the
 *              call would share an address (a item_stride = b t_stride for some 0 <= a < n, 0 <= b < l, not both zero: rows (l, 1) and domain order
 *              (1, n) never do), (n - 1) item_stride or (l - 1) t_stride of 2^47 or more -> KEAKI_ERR_BAD_ARG; l > len(srs_g1) -> KEAKI_ERR_TOO_LARGE; a refused workspace ->
 *              KEAKI_ERR_OOM. Nothing is written in any of these cases, nothing is launched, and the context stays usable.
 *   kernels    csrc/kzg_cosets.hip: one launch derives 1 / h_k, s_k = gamma_k c_k and sum gamma; one launch runs the size-l inverse transforms of ALL
 *              items in LDS (tiles of 1024 / l items, (l / 2) log2 l butterflies per item, twist and gamma applied before the sum over items), a
 *              third folds the per-workgroup rows into -J. Then: MSM of gamma over the proofs (R), MSM of s over the proofs, MSM of -J over
 *              [tau^j]_1, MSM of gamma over the commitments (or (sum gamma) C), one sum, ONE launch of two pairings.
 *   host form  one upload in front of the kernels (the span of the values the strides name; no chunk pipeline), the kernels, 896 bytes back;
 *              returns only when nothing reads or writes caller memory, also on failure.
 *   _dev       every array is a device pointer (16-byte aligned; the commitment, [tau^l]_2 and omega too); omega_l_inv, inv_l (read before the call
 *              returns), ok_out and sums_out_aff stay HOST pointers, so this form synchronises as well. Workspace: 64 B per item + 32 B per value
 *              of at most 1,024 tiles, grow-only, counted in keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim.
 *   out of scope  The multi-GPU form: the host layers refuse a device group. (The per-coset verdict is keaki_hip_kzg_verify_cosets_each, below.)
 *   numbers    (MI355X, medians of alternating rounds in one process: profiles/verify_cosets_times.txt, bench_tools/bench_verify_cosets.py) all r cosets of a
 *              vector, resident / from host arrays, l = 4 / 16 / 64: d = 2^20 7.8 / 7.4 / 7.2 ms (host 8.7 / 8.2 / 8.0), 2^16 7.0 / 6.9 / 7.1, 2^12 6.9 / 7.2 /
 *              7.1; l = 1,024 at d = 2^20 7.6 ms (8.2). Against (a) the only route before, r calls of keaki_hip_kzg_verify_multi (7.7 - 8.8 ms each at l <=
 *              64, 23 at l = 1,024; 64 calls timed, EXTRAPOLATED to r): 126 s at d = 2^20, l = 64 (1/17,600), 2,275 s at l = 4; at r = 2, measured, 7.7 ms
 *              against 15.6 - 47: the call wins from r = 2 on at every shape. Against (b) keaki_hip_kzg_verify_batch_dev on the same d values as d single
 *              openings (which needs d proofs, not r): 9.1 - 9.2 ms at d = 2^20 (the call takes 0.78 - 0.86 of it), 6.4 - 6.5 at 2^16 and 6.2 - 6.3 at 2^12, where
 *              the call LOSES by 0.4 - 0.9 ms (1.05 - 1.15 x): both are floors of launches there, and this call has one MSM and the inversion chain more.
 *              The Fr kernels at d = 2^20, l = 4 / 64 / 1,024: k_vc_prepare 0.52 / 0.56 / 0.61 ms (ONE Fermat chain's latency, whatever n is), k_vc_transform
 *              0.06 / 0.12 / 0.23 ms, k_vc_finish 0.10 / 0.08 / 0.08 ms: a tenth of the call; the rest is the MSMs' and the pairings' (1.46 ms). */
keaki_status keaki_hip_kzg_verify_cosets(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride,
                                         const uint64_t* tau_l_g2_aff, const uint64_t* points, int32_t point_mode, const uint64_t* values,
                                         size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l,
                                         const uint64_t* proofs_aff, const uint64_t* gammas, size_t n, int32_t* ok_out, uint64_t* sums_out_aff);
keaki_status keaki_hip_kzg_verify_cosets_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride,
                                             const void* d_tau_l_g2_aff, const void* d_points, int32_t point_mode, const void* d_values,
                                             size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv,
                                             const uint64_t* inv_l, const void* d_proofs_aff, const void* d_gammas, size_t n, int32_t* ok_out,
                                             uint64_t* sums_out_aff);

/* ---- KZG set batch verification: n set proofs over ARBITRARY point sets of one size in one call -------------------------------------------------
 * What keaki_hip_kzg_verify_multi checks one proof at a time, for n items at once, the sets being any k distinct points each (the proofs that
 * kzg::open_set, kzg::aggregate_proofs and vec::vec_open_subset hand out; cosets of one size are keaki_hip_kzg_verify_cosets' case). Item i < n: a
 * commitment C_i, the k points z_(i,0) .. z_(i,k-1), the k claimed values y_(i,j) = p_i(z_(i,j)), a proof pi_i, the caller's coefficient gamma_i.
 *     Z_i(X) = prod_j (X - z_(i,j)) = sum_(t <= k) Z_(i,t) X^t  (monic: Z_(i,k) = 1)       I_i(X) = sum_(t < k) I_(i,t) X^t, the interpolant of (z_(i,j), y_(i,j))
 * The single check e(C_i - [I_i(tau)]_1, g2) == e(pi_i, [Z_i(tau)]_2) has the right side prod_t e(Z_(i,t) pi_i, [tau^t]_2): the sets differ, so no one
 * G2 point serves all items, but the COEFFICIENTS of Z cross the pairing as G1 scalars, and [tau^0]_2 = g2 folds into the left side.
 * The call evaluates EXACTLY this combination:
 *     J_t = sum_i gamma_i I_(i,t)  (t < k)       L = sum_i gamma_i C_i - sum_t J_t [tau^t]_1 - sum_i (gamma_i Z_(i,0)) pi_i
 *     R_t = sum_i (gamma_i Z_(i,t)) pi_i  (1 <= t <= k;  R_k = sum_i gamma_i pi_i)
 *     *ok_out = 1  <=>  e(-L, g2) prod_(t = 1 .. k) e(R_t, [tau^t]_2) == 1
 * for the gammas it is given; that is a deterministic contract. If all n items are valid it always accepts. If one is invalid it rejects except
 * with probability <= 1/r -- PROVIDED the gamma_i are independent, uniform in Fr and unknown to whoever produced the proofs. Badly chosen gammas
 * void the bound: with all gamma_i equal, two errors can cancel, and gamma = 0 accepts anything. gammas are drawn by the caller, one Fr::rand per item
 * in index order (the rule encap_batch follows for r), so the randomness stream stays the caller's and every result is reproducible. At k = 1 the
 * equation is keaki_hip_kzg_verify_batch's (Z = X - z: -gamma Z_0 = gamma z, J_0 = sum gamma y, [tau^0]_1 = g1): sums_out_aff is byte for byte what that
 * call returns.
 *   srs_g1, srs_g2   srs_g1 is read at its points 0 .. k - 1 ([tau^t]_1, through its window tables where it has them), srs_g2 at its points 1 .. k ([tau^t]_2,
 *                as keaki_hip_kzg_verify_multi reads it)
 *   com_aff      com_stride = 0: ONE affine G1 point u64[8], the commitment of all items (subsets of one vector); 1: n points
 *   points       point_mode = 0: Fr, item i's point j at word 4 (i item_stride + j). 1: u32 domain indices at the same ELEMENT offsets (index (i, j) is
 *                the u32 at points + 4 (i item_stride + j) bytes) and omega ONE Fr: z = omega^idx, derived on the device (what vec_verify_subsets needs).
 *                omega is NULL in point_mode 0.
 *   values       value (i, j) is the Fr at word 4 (i item_stride + j); item_stride >= k, the gap between two rows is never read
 *   proofs_aff, gammas   n affine G1 points, n Fr
 *   sums_out_aff (k + 1) x u64[8] = L, then R_1 .. R_k, affine ((0,0) = identity): what the Miller loops ran on, before L is negated; or NULL
 *   repeated point   two equal points within an item are no set. The library does NOT look: a repeated point zeroes a weight -- and the weights of the up to
 *                16 (item, point) pairs that share its inversion -- and the results are meaningless. Distinct points are the caller's contract, exactly as
 *                for keaki_hip_kzg_set_polys; the host layers (host/keaki.cpp, rust/keaki/src/hip.rs) refuse repeats.
 * Identity commitments and proofs, zero values and gammas are ordinary inputs. n = 0: *ok_out = 1, the sums are the identity.
 *   errors     a null required pointer, k = 0 or k > KEAKI_VERIFY_SETS_K_MAX, item_stride < k, com_stride or point_mode outside {0, 1}, n k >= 2^31 (or n >=
 *              2^31), (n - 1) item_stride of 2^47 or more, point_mode 1 without omega -> KEAKI_ERR_BAD_ARG; k + 1 > len(srs_g2) or k > len(srs_g1) ->
 *              KEAKI_ERR_TOO_LARGE; a refused workspace -> KEAKI_ERR_OOM. Nothing is written in any of these cases, nothing is launched, and the context
 *              stays usable.
 *   kernels    csrc/kzg_sets.hip: (point_mode 1) one launch derives the points; one launch the weights 1 / Z_i'(z_(i,j)) (k - 1 products per pair, ONE Fermat
 *              inversion per 16 pairs); one launch Z_i and I_i of ALL items in LDS (tiles of 256 / kp items, kp = the power of two >= k; O(k^2) products per
 *              item), the k + 1 scalar rows and the per-workgroup sums of gamma I; a fourth folds those into -J and sum gamma. Then: the batched MSM
 *              of the k + 1 rows over the proofs (rows of more than 16,384 items: one MSM per row), the MSM of -J over [tau^t]_1, the MSM of gamma over the
 *              commitments (or (sum gamma) C), one sum, k + 1 Miller loops, their product (csrc/gt_product.hip) and ONE final exponentiation:
 *              keaki_hip_pairing_product, below. 384 GT bytes come back and are compared with GT one on the host. Nothing here is n pairings or in G2.
 *   host form  one upload in front of the kernels (the spans of the points and values the stride names; no chunk pipeline), the kernels, 384 bytes
 *              (+ 64 (k + 1)) back; returns only when nothing reads or writes caller memory, also on failure.
 *   _dev       every array is a device pointer (16-byte aligned; 4-byte for the indices of point_mode 1); omega (read before the call returns), ok_out and
 *              sums_out_aff stay HOST pointers, so this form synchronises as well. Workspace: 32 (2 k + 1) B per item (32 (3 k + 1) in point_mode 1) + 32
 *              (k + 1) B per tile of at most 1,024 + 24 KB + the batched MSM's, grow-only, counted in keaki_hip_ctx_memory out4[1], released by
 *              keaki_hip_ctx_trim.
 *   out of scope  k > 64; a G2-side route for few items with large sets; the multi-GPU form (the host layers refuse a
 *              device group). Items of unequal k are grouped by k, one call per size, by the host layers. The per-item verdict is
 *              keaki_hip_kzg_verify_sets_each, below.
 *   numbers    (MI355X, medians of alternating rounds in one process: profiles/verify_sets_times.txt, bench_tools/bench_verify_sets.py) resident / from host
 *              arrays, one commitment per item, k = 2 / 8 / 64: n = 2 6.6 / 6.7 / 8.3 ms, n = 64 6.4 / 6.6 / 7.9, n = 4,096 6.4 / 6.9 / 11.1 (host 6.6 / 7.0 / 11.4),
 *              n = 2^16 10.3 / 22.5 / 153.7 (host 10.6 / 23.4 / 158.6), n = 2^20 15.6 / 41.2 ms at k = 2 / 8 (host 21.0 / 53.8). Against (a) the only route before, n
 *              calls of keaki_hip_kzg_verify_multi (7.6 - 8.9 ms each; 64 calls timed, EXTRAPOLATED beyond): the call wins at every shape, from n = 1 on (n = 1,
 *              measured: 5.0 / 5.1 / 7.2 ms against 8.4 / 8.9 / 7.6; n = 2: 6.4 / 6.6 / 8.7 against 16.6 / 17.0 / 15.3; n = 2^16, k = 8: 22.5 ms against 570 s): the k + 1
 *              Miller loops run side by side and share one final exponentiation, so they do not make small n lose. Against (b) keaki_hip_kzg_verify_cosets_dev
 *              on coset-shaped inputs of the same n and k, the floor: 0.74 - 0.99 of its time up to n = 4,096 at k <= 8 and n = 64 at k = 64, and it LOSES beyond:
 *              n = 4,096, k = 64 1.38 x; n = 2^16 1.25 / 2.67 / 17.4 x; n = 2^20 1.31 / 3.35 x -- rows of more than 16,384 items leave the batched MSM and cost one
 *              full MSM each (k + 1 of them), and the polynomial kernel's n k^2 products show at k = 64. The kernels at n = 2^16, k = 2 / 8 / 64: k_vs_weights 0.44 /
 *              0.59 / 5.66 ms, k_vs_polys 0.03 / 0.30 / 18.1 ms, k_vs_finish 0.02 / 0.03 / 0.06 ms, k_gt_product 0.11 / 0.11 / 0.18 ms; the Miller loops 0.70 - 0.72 ms,
 *              the final exponentiation 0.76 - 0.77 ms. There is no route switch. */
keaki_status keaki_hip_kzg_verify_sets(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                       int32_t com_stride, const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values,
                                       size_t item_stride, size_t k, const uint64_t* proofs_aff, const uint64_t* gammas, size_t n, int32_t* ok_out,
                                       uint64_t* sums_out_aff);
keaki_status keaki_hip_kzg_verify_sets_dev(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs_g1, const keaki_hip_srs_g2* srs_g2, const void* d_com_aff,
                                           int32_t com_stride, const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values,
                                           size_t item_stride, size_t k, const void* d_proofs_aff, const void* d_gammas, size_t n, int32_t* ok_out,
                                           uint64_t* sums_out_aff);

/* ---- pairing product: prod_i e(g1[i], g2[i]) with ONE final exponentiation ------------------------------------------------------------------------
 * gt_out = the 384 bytes of serialize_uncompressed(prod_(i < n) e(g1[i], g2[i])): n Miller loops, a product tree over their outputs (csrc/gt_product.hip:
 * the elements in the representation keaki_hip_miller_loop_batch documents, multiplied by the pairing kernels' own Fq12 product; a second launch when n
 * exceeds one workgroup's share of 128), ONE final exponentiation. An identity in either slot contributes GT one; n = 0 gives GT one. n < 2^31.
 *   errors     a null required pointer (gt_out at any n; the point arrays for n > 0), n >= 2^31 -> KEAKI_ERR_BAD_ARG; a refused workspace -> KEAKI_ERR_OOM;
 *              nothing is written then.
 *   _dev       device pointers (d_gt_out: 384 bytes, 16-byte aligned); asynchronous on the context's stream. Workspace: 384 B per pair + 96 KB, grow-only,
 *              counted in keaki_hip_ctx_memory out4[1], released by keaki_hip_ctx_trim. */
keaki_status keaki_hip_pairing_product(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, size_t n, uint8_t* gt_out);
keaki_status keaki_hip_pairing_product_dev(keaki_hip_ctx* ctx, const void* d_g1_aff, const void* d_g2_aff, size_t n, void* d_gt_out);

/* ---- KZG coset pairs and per-coset verdicts: the per-item side of the coset check, all n cosets in one call -----------------
 * verify_cosets answers "are all n set proofs valid?" in two pairings. Two things need the PER-ITEM points of the same check
 *     e(A_k, g2) == e(pi_k, [tau^l]_2 - c_k g2)        A_k = C_k - [I_k(tau)]_1        c_k = h_k^l
 * (I_k the coset interpolant defined above): a verdict per coset, and encryption to the claimed values of every coset (ct_k = r_k ([tau^l]_2 - c_k g2),
 * key_k = KDF(e(r_k A_k, g2)): keaki_hip_encap_multi / _encrypt_multi with n groups of one item, coms := A, points := c, values := 0 and [tau^l]_2).
 *
 * keaki_hip_kzg_coset_pairs: lhs_out_aff[k] = A_k (affine G1, (0,0) = identity), c_out[k] = c_k (Fr, Montgomery).
 *   srs_g1, com_aff, com_stride, points, point_mode, values, item_stride, t_stride, log2l, omega_l_inv, inv_l, n, the zero-shift rule
 *              exactly as in keaki_hip_kzg_verify_cosets. The handle is not const: its coset table is built on first use (below).
 *   equalities lhs_out_aff[k] followed by [tau^l]_2 - c_k g2 is pair_out_aff of keaki_hip_kzg_verify_multi on the l points h_k omega_l^t of coset k.
 *              Every route, and handles with and without window tables or a precomputed coset table, give the same bytes (affine points are unique).
 *   errors     those of keaki_hip_kzg_verify_cosets (a null required pointer, com_stride or point_mode outside {0, 1}, l > KEAKI_SET_MAX, n l >= 2^31,
 *              overlapping strides, extents of 2^47 -> KEAKI_ERR_BAD_ARG; l > len(srs_g1) -> KEAKI_ERR_TOO_LARGE; a refused workspace -> KEAKI_ERR_OOM): nothing
 *              is written, nothing launched, the context stays usable. n = 0: nothing is written.
 *   kernels    csrc/kzg_cosets.hip, the instantiations without gammas of verify_cosets' kernels: 1 / h_k and c_k (one Fermat inversion per 16 items), then
 *              per launch chunk the size-l inverse transforms in LDS with EVERY item's row -a_(k,j) stored (32 B per value). csrc/kzg_coset_pairs.hip:
 *              route 1, k_cp_rows: all rows share the l bases [tau^j]_1, so the handle keeps T[j][w][d] = d 2^(wb w) [tau^j]_1 (signed wb-bit digits, wb =
 *              13 / 10 / 8 bits for l <= 64 / <= 512 / 1,024: the widest whose table stays under 512 MiB, csrc/coset_rows_plan.h) and a row is l x ceil(254 / wb)
 *              additions in the lazy 29-bit XYZZ form with no doublings (l = 64: 1,280 against about 5,300 of the batched MSM; l = 4: 80 against about
 *              1,450). A lane owns an (item, slice of the l bases); the S slices of an item (S a power of two <= min(l, 64), doubled while the launch has
 *              fewer than "coset_rows_min_lanes" lanes) meet by cross-lane exchange; one general addition joins C_k; k_cp_affine inverts 8 items under
 *              one inversion. Route 2: the rows through the batched MSM (keaki_hip_msm_g1_batch's kernels) plus C_k: the fallback when the table's
 *              allocation is refused, and the A/B partner ("coset_rows_route").
 *   table      64 B x l x windows x (2^(wb - 1) + 1): 21 MB at l = 4, 336 MB at l = 64, 437 MB at l = 512, 270 MB at l = 1,024. Built on first use or by
 *              keaki_hip_srs_g1_precompute_cosets, cached in the SRS handle for ONE l beside the FK23, update and FK23-coset caches (none evicts another),
 *              counted in keaki_hip_ctx_memory out4[0], freed with the handle. Results never depend on it.
 *   chunks     launch chunks of at most 2^20 values (32 MiB of rows + 224 B per item), grow-only, counted in out4[1]; a refused reservation halves the
 *              chunk, and the call fails only when one item does not fit. + 32 B per item of the call (1 / h_k).
 *   host form  one upload in front (the span of the values the strides name), the kernels, one download of 96 n bytes; returns only when nothing reads or
 *              writes caller memory, also on failure.
 *   _dev       every array is a device pointer (16-byte aligned; the commitment and omega too); omega_l_inv, inv_l stay HOST pointers, read before the
 *              call returns. Asynchronous on the context's stream.
 *
 * keaki_hip_kzg_verify_cosets_each: status[k] = 0 <=> the coset check holds for item k. With c_k pi_k moved across the pairing:
 *     L_k = A_k + c_k pi_k          status[k] = 0  <=>  e(L_k, g2) * e(-pi_k, [tau^l]_2) == 1
 * which is keaki_hip_kzg_verify_each on (coms := A, points := c, values := 0, [tau]_2 := [tau^l]_2): coset_pairs into the workspace, then that call's
 * kernels unchanged (no new pairing code). The verdict is exact and equals that of keaki_hip_kzg_verify_multi on the l points of item k; n_bad = 0 <=>
 * keaki_hip_kzg_verify_cosets accepts (for any gammas with valid items; with the probability stated there otherwise). At log2l = 0 the status and L bytes
 * are those of keaki_hip_kzg_verify_each with z_k = h_k.
 *   tau_l_g2_aff, proofs_aff   as in keaki_hip_kzg_verify_cosets;   status, n_bad, first_bad, lhs_out_aff (the L_k, or NULL), identities, [tau^l]_2 = identity,
 *              n = 0 and "a bad item never fails the call" as in keaki_hip_kzg_verify_each; errors: those of both calls, nothing written.
 *   workspace  + 128 B per item of the call (A_k, c_k, the zero values) on top of both calls' own.
 *   _dev       n_bad and first_bad stay HOST pointers: synchronises, like keaki_hip_kzg_verify_each_dev.
 *   out of scope  device groups / multi-GPU (the host layers refuse a device group), and a C-ABI encap_cosets: encryption to cosets is composed from
 *              keaki_hip_kzg_coset_pairs and keaki_hip_encap_multi / keaki_hip_encrypt_multi by the caller.
 *   numbers    (MI355X, medians of alternating rounds in one process: profiles/coset_each_times.txt, bench_tools/bench_coset_each.py) all r cosets of a vector,
 *              l = 4 / 16 / 64. coset_pairs resident, route 1: d = 2^20 2.8 / 3.1 / 3.2 ms (4.4 / 3.8 / 3.8 from host arrays), 2^16 0.88 / 0.87 / 1.04, 2^12 0.78 /
 *              0.92 / 0.96; l = 1,024 at 2^20 5.1 ms. Route 2 on the same inputs: 173 / 50 / 18 ms at 2^20 (13 at l = 1,024), 11.5 / 5.0 / 3.3 at 2^16, 2.8 / 2.4 /
 *              2.5 at 2^12: the table route wins at EVERY measured shape (2.6 - 62 x) and is the default at every l. verify_cosets_each resident: d = 2^20 43.2 /
 *              13.7 / 9.0 ms (10.7 at l = 1,024), 2^16 and 2^12 6.4 - 6.7 ms (the latency of one pairing chunk); keaki_hip_kzg_verify_cosets on the same items,
 *              the floor: 7.0 - 7.6 ms. Against the only route before, r calls of keaki_hip_kzg_verify_multi (64 timed at 7.7 - 8.8 ms each, 23 ms at l = 1,024,
 *              EXTRAPOLATED to r): 125 s at d = 2^20, l = 64 (1/14,000), 2,251 s at l = 4 (1/52,000). Encryption to all cosets through the host layer
 *              (vec_encrypt_cosets, 32-byte messages) at d = 2^16: 13.3 / 5.7 / 3.9 ms against 276 / 69 / 16 s as r encrypt_set calls (64 timed, EXTRAPOLATED).
 *              The width and lane sweeps behind the plan are in the same file and summarised in csrc/coset_rows_plan.h. Kernel shares (rocprofv3) and the
 *              first call's table build were not measured. */
keaki_status keaki_hip_srs_g1_precompute_cosets(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs, uint32_t log2l);
keaki_status keaki_hip_kzg_coset_pairs(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride, const uint64_t* points,
                                       int32_t point_mode, const uint64_t* values, size_t item_stride, size_t t_stride, uint32_t log2l,
                                       const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, uint64_t* lhs_out_aff, uint64_t* c_out);
keaki_status keaki_hip_kzg_coset_pairs_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride, const void* d_points,
                                           int32_t point_mode, const void* d_values, size_t item_stride, size_t t_stride, uint32_t log2l,
                                           const uint64_t* omega_l_inv, const uint64_t* inv_l, size_t n, void* d_lhs_out_aff, void* d_c_out);
keaki_status keaki_hip_kzg_verify_cosets_each(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const uint64_t* com_aff, int32_t com_stride,
                                              const uint64_t* tau_l_g2_aff, const uint64_t* points, int32_t point_mode, const uint64_t* values,
                                              size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv, const uint64_t* inv_l,
                                              const uint64_t* proofs_aff, size_t n, uint8_t* status, uint64_t* n_bad, uint64_t* first_bad,
                                              uint64_t* lhs_out_aff);
keaki_status keaki_hip_kzg_verify_cosets_each_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, const void* d_com_aff, int32_t com_stride,
                                                  const void* d_tau_l_g2_aff, const void* d_points, int32_t point_mode, const void* d_values,
                                                  size_t item_stride, size_t t_stride, uint32_t log2l, const uint64_t* omega_l_inv,
                                                  const uint64_t* inv_l, const void* d_proofs_aff, size_t n, void* d_status, uint64_t* n_bad,
                                                  uint64_t* first_bad, void* d_lhs_out_aff);

/* ---- KZG set pairs and per-set verdicts: the per-item side of the set check over ARBITRARY point sets, all n items in one call ------------------
 * verify_sets answers "are all n set proofs valid?"; these calls give the PER-ITEM points of the same check
 *     e(A_i, g2) == e(pi_i, Z2_i)        A_i = C_i - [I_i(tau)]_1  (G1)        Z2_i = [Z_i(tau)]_2  (G2)
 * (Z_i, I_i the vanishing polynomial and the interpolant of item i, as for keaki_hip_kzg_verify_sets): a verdict per item, and encryption to the claimed
 * values of every item (ct_i = r_i Z2_i, key_i = KDF(e(r_i A_i, g2)): keaki_hip_encap_multi / _encrypt_multi with n groups of one item, coms := A, points =
 * values = 0, then keaki_hip_g2_mul_batch over the Z2_i).
 *
 * keaki_hip_kzg_set_pairs: lhs_out_aff[i] = A_i (affine G1, u64[8]), z2_out_aff[i] = Z2_i (affine G2, u64[16]); (0,0) = identity in both.
 *   com_aff, com_stride, points, point_mode, omega, values, item_stride, k, n, the limits (k <= KEAKI_VERIFY_SETS_K_MAX, n k < 2^31) and the repeated-point rule
 *   are keaki_hip_kzg_verify_sets'. srs_g1 is read at its points 0 .. k - 1, srs_g2 at 0 .. k; both handles are non-const: each keeps a window table that is built
 *   on first use (srs_g1: the table of keaki_hip_kzg_coset_pairs at l = kp, the power of two >= k; srs_g2: below).
 *   equalities lhs_out_aff[i] followed by z2_out_aff[i] is byte for byte the pair_out_aff of keaki_hip_kzg_verify_multi on item i (affine points are unique
 *              encodings). At k = 1: A_i = C_i - y_i g1, Z2_i = [tau]_2 - z_i g2.
 *   identities an identity commitment and zero values are ordinary inputs; A_i can be the identity, and Z2_i too (tau inside the point set: reachable with a
 *              structured SRS).
 *   errors     those of keaki_hip_kzg_verify_sets: a null required pointer, k = 0 or k > KEAKI_VERIFY_SETS_K_MAX, item_stride < k, a flag outside {0, 1},
 *              point_mode 1 without omega, n k >= 2^31, extents of 2^47 -> KEAKI_ERR_BAD_ARG; k + 1 > len(srs_g2) or k > len(srs_g1) -> KEAKI_ERR_TOO_LARGE; a
 *              refused workspace, or a G2 table refused at all three widths -> KEAKI_ERR_OOM. Nothing is written in any of these cases, nothing is launched,
 *              and the context stays usable. n = 0: KEAKI_OK, nothing is written.
 *   kernels    per launch chunk (csrc/set_rows_plan.h). Fr side, csrc/kzg_sets.hip: k_vs_points (point_mode 1), k_vs_weights, then the rows instantiation of
 *              k_vs_polys (no gammas, no partial sums, no k_vs_finish): -I_(i,t) padded with zeros to kp at (i << log2 kp) + t, and Z_(i,t), t < k (Z is monic:
 *              the coefficient of X^k is not stored). G1 side: the group side of keaki_hip_kzg_coset_pairs at log2l = log2 kp -- k_cp_rows over the G1 handle's
 *              window table (zero digits are skipped: the padding costs loads only), k_cp_affine; the batched MSM + k_cp_join when that table is refused or
 *              kp > len(srs_g1) >= k; "coset_rows_route" / "coset_rows_wb" / "coset_rows_min_lanes" keep their meaning. G2 side, csrc/kzg_set_pairs.hip:
 *              k_sp_rows_g2 -- a lane owns (item, slice of the k bases), walks the signed wb-bit digits of its Z coefficients (carry included) and adds the
 *              entries of the G2 handle's window table T2[j][w][d] = d 2^(wb w) [tau^j]_2 (affine, 128 B, base-major: a table of kb bases serves every k <=
 *              kb) into a lazy-limb XYZZ accumulator with the complete addition (equal operands double, opposite ones give the identity and the walk goes
 *              on, identity entries are skipped); the S slices of an item meet by cross-lane exchange in a wave, slice 0 adds [tau^k]_2. No doublings: a row
 *              is k x ceil(254 / wb) G2 additions. k_sp_affine_g2: four items per lane under ONE Fq2 inversion.
 *   table      built on first use or by keaki_hip_srs_g2_precompute_sets(ctx, srs, k_max) (k_max bases at the plan's width), cached in the G2 handle until a
 *              larger k or another width arrives, counted in keaki_hip_ctx_memory out4[0], freed with the handle. With "set_rows_wb" = 0 a resident table that
 *              covers k is used at the width it HAS: a handle first used at k = 64 (10 bits) or under a forced width keeps that width for smaller k, so
 *              the plan's width holds for the first k of a handle (or the k_max of _precompute_sets), not for every later call. Width: "set_rows_wb" (8, 10 or 13), 0 = by plan
 *              (csrc/set_rows_plan.h: the widest of 13 / 10 / 8 bits whose table stays under 512 MiB: 10.5 MB / 1.7 MB / 0.53 MB per base, so 13 bits up to
 *              k = 51 and 10 bits beyond; the wider table won at every measured shape -- see that header). A refused table falls to the next narrower width,
 *              then KEAKI_ERR_OOM. "set_rows_min_lanes": the slice threshold (1 .. 2^31, 0 = the built-in 65,536, measured). Results do not depend on either; other values are refused with KEAKI_ERR_BAD_ARG, in the
 *              environment ignored.
 *   host form  one upload in front (the spans of points and values the stride names, through the family's stager), the kernels, one download; returns only
 *              when nothing reads or writes caller memory, also on failure.
 *   _dev       device pointers (16-byte aligned; 4-byte for the indices of point_mode 1); omega stays a HOST pointer, read before the call returns.
 *              Asynchronous on the context's stream. Workspace: per item of a launch chunk 32 (kp + 2 k) B (+ 32 k in point_mode 1) + 384 B (+ 96 B on the MSM
 *              route), grow-only, counted in out4[1], released by keaki_hip_ctx_trim.
 *
 * keaki_hip_kzg_verify_sets_each: status[i] = 0 <=> keaki_hip_kzg_verify_multi accepts item i; *n_bad = 0 <=> keaki_hip_kzg_verify_sets accepts (valid items, any
 * gammas). At k = 1 the bytes are keaki_hip_kzg_verify_each's. With R_i = (pi_i is the identity or Z2_i is the identity): if A_i or R_i is an identity, the
 * item is valid iff both are; no arithmetic decides such an item. A bad item never fails the call. lhs_out_aff / z2_out_aff (or NULL): the pairs the verdicts
 * were computed from. n = 0: *n_bad = 0, *first_bad = UINT64_MAX, nothing else is written. Errors: those above; status, n_bad required.
 *   kernels    set_pairs into the workspace, then per launch chunk (as keaki_hip_kzg_verify_each: at most 2^16 items, halved on a refused reservation down
 *              to 32) the verdicts, then k_ve_count. "set_each_route" = 1: csrc/kzg_set_each_pair.hip, k_pairing2v, one lane pair per item: a Miller
 *              step squares f ONCE, multiplies by the tabulated line of g2 at A_i and by the on-the-fly line of the running point T (from Z2_i) at -pi_i -- 64
 *              squarings for the two pairings together -- then ONE final exponentiation and the comparison with one; one status byte. = 2: existing kernels
 *              -- the Miller loops of (A_i, g2) and (-pi_i, Z2_i) in one launch, a pairwise product (csrc/gt_product.hip: k_gt_pair_product), the final
 *              exponentiation, a comparison of the 384 bytes with GT one (k_sp_status). The two routes agree to the byte. 0 = by plan, which is route 2 at
 *              every n: MEASURED, the fused kernel lost at every size but one (n = 32,768) and by 23 % at n = 2^20; it stays as the A/B form.
 *   _dev       n_bad, first_bad and omega stay HOST pointers: this form synchronises, like keaki_hip_kzg_verify_each_dev.
 *   out of scope  a C-ABI encapsulation to sets (compose as above); k > 64; device groups and the multi-GPU form.
 *   numbers    (MI355X, medians of alternating rounds in one process: profiles/set_each_times.txt, bench_tools/bench_set_each.py) one commitment per item, k = 2 /
 *              8 / 64. set_pairs resident: n = 2 1.00 / 1.31 / 3.11 ms, n = 64 1.23 / 1.34 / 3.00, n = 4,096 1.13 / 1.39 / 5.35, n = 2^16 1.61 / 4.53 / 54.8 (from host
 *              arrays 2.44 / 5.95 / 60.7). verify_sets_each resident, by plan: n = 2 2.5 / 2.9 / 4.4 ms, n = 64 2.7 / 2.9 / 4.5, n = 4,096 4.8 / 4.9 / 8.8, n = 2^16 16.4 /
 *              18.3 / 68.2. Against n calls of keaki_hip_kzg_verify_multi (7.7 - 8.7 ms each; 64 timed, EXTRAPOLATED beyond): it wins at every shape, 3.6 - 6.7 x at
 *              n = 2, 109 - 207 x at n = 64, 7,400 - 34,000 x at n = 2^16. Against keaki_hip_kzg_verify_sets_dev on the same items (ONE verdict, the floor) it
 *              is FASTER up to n = 4,096 (0.39 - 0.79 of its time: that call's k + 1 Miller loops and MSMs have a floor of 6.4 ms) and at n = 2^16, k = 8 / 64
 *              (0.82 / 0.45), and LOSES at n = 2^16, k = 2 (1.6 x). Against keaki_hip_kzg_verify_cosets_each_dev on coset-shaped inputs it is faster up to
 *              n = 64 and at n = 4,096, k <= 8 (0.39 - 0.76) and LOSES at n = 4,096, k = 64 (1.20 x) and at n = 2^16 (1.27 / 1.33 / 3.0 x): Z2_i costs k x 20 - 26
 *              G2 additions per item where the cosets share ONE G2 point. Encryption to sets (host mirror: enc::encrypt_sets, vec::vec_encrypt_subsets) is
 *              tested, NOT measured. */
keaki_status keaki_hip_srs_g2_precompute_sets(keaki_hip_ctx* ctx, keaki_hip_srs_g2* srs, size_t k_max);
keaki_status keaki_hip_kzg_set_pairs(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff, int32_t com_stride,
                                     const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values, size_t item_stride, size_t k,
                                     size_t n, uint64_t* lhs_out_aff, uint64_t* z2_out_aff);
keaki_status keaki_hip_kzg_set_pairs_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const void* d_com_aff, int32_t com_stride,
                                         const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values, size_t item_stride, size_t k,
                                         size_t n, void* d_lhs_out_aff, void* d_z2_out_aff);
keaki_status keaki_hip_kzg_verify_sets_each(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const uint64_t* com_aff,
                                            int32_t com_stride, const void* points, int32_t point_mode, const uint64_t* omega, const uint64_t* values,
                                            size_t item_stride, size_t k, const uint64_t* proofs_aff, size_t n, uint8_t* status, uint64_t* n_bad,
                                            uint64_t* first_bad, uint64_t* lhs_out_aff, uint64_t* z2_out_aff);
keaki_status keaki_hip_kzg_verify_sets_each_dev(keaki_hip_ctx* ctx, keaki_hip_srs_g1* srs_g1, keaki_hip_srs_g2* srs_g2, const void* d_com_aff,
                                                int32_t com_stride, const void* d_points, int32_t point_mode, const uint64_t* omega, const void* d_values,
                                                size_t item_stride, size_t k, const void* d_proofs_aff, size_t n, void* d_status, uint64_t* n_bad,
                                                uint64_t* first_bad, void* d_lhs_out_aff, void* d_z2_out_aff);

/* ---- KZG verify_each: one verdict per opening, n openings in one call ---------------------------------------------------
 * verify_batch answers "are all n openings valid?"; this call says WHICH are not. Per item, by bilinearity (z_i proof_i moved across the
 * pairing, as in verify_batch):
 *     L_i = C_i - y_i g1 + z_i proof_i          status[i] = 0  <=>  e(L_i, g2) * e(-proof_i, [tau]_2) == 1
 * Both second arguments are fixed for the call, so both line sequences are tables ([tau]_2's is built on first use and kept in the context
 * until another [tau]_2 arrives); the two Miller loops share their 64 squarings and ONE final exponentiation, and the result is compared with
 * one on the device. The verdict is exact -- no gammas, no error probability -- and always equals that of keaki_hip_kzg_verify on the item.
 *   com_aff, com_stride, tau_g2_aff, points, point_mode, values, proofs_aff     exactly as in keaki_hip_kzg_verify_batch
 *   status       n bytes: 0 = the equation holds (accepted, as in _decompress), 1 = it does not
 *   n_bad        the number of ones (required);   first_bad   index of the first one, UINT64_MAX if none (may be NULL)
 *   lhs_out_aff  n affine G1 points L_i ((0,0) = identity), or NULL: what the first pairing slot was evaluated on
 * Identities are ordinary inputs: L_i and proof_i both the identity is valid (a constant polynomial: C = y g1, proof = 0), exactly one of them
 * is invalid; [tau]_2 = identity: valid_i <=> L_i is the identity. Points are assumed to be on the curve (decode untrusted ones with
 * _decompress first). A bad item never fails the call.
 * n = 0: *n_bad = 0, *first_bad = UINT64_MAX, nothing else written. com_stride or point_mode outside {0, 1}, a null required pointer with n > 0,
 * n >= 2^31: KEAKI_ERR_BAD_ARG, nothing written.
 * Host form: one upload in front, the kernels in launch chunks of at most 2^17 items, one download of n bytes (+ 64 n with lhs_out_aff); no
 * chunk pipeline -- the inputs are at most 192 B per item against >= 140 ns of pairing work per item, a few per cent. The call returns when
 * nothing reads or writes caller memory any more, also on failure.
 * _dev: every array is a device pointer (the commitment, [tau]_2 and omega too); n_bad and first_bad stay HOST pointers, so this form
 * synchronises, like _decompress_dev.
 * Workspace: 3,968 B per item of a launch chunk, grow-only; a refused reservation halves the chunk, and the call fails (the context stays
 * usable) only when 32 items do not fit.
 * Measured (profiles/verify_each_times.txt, resident, medians of alternating rounds in one process): 2^16 items 10.5 ms, 2^20 items 156.7 ms
 * (160.5 ms from host arrays). Against ONE pairing with lines on the fly per item (keaki_hip_pairing_batch_dev over n items): 1.15 x / 1.13 x
 * its time at 2^16 / 2^20 (0.57 x / 0.56 x the time of two), 3.97 x at 2^10 where the call is one lane-pair pairing's latency (6.1 ms).
 * Against n single keaki_hip_kzg_verify calls, EXTRAPOLATED from the mean of 64 (1.68 ms): 1/284 at 2^10, 1/10,500 at 2^16, 1/11,300 at 2^20. */
keaki_status keaki_hip_kzg_verify_each(keaki_hip_ctx* ctx, const uint64_t* com_aff, int32_t com_stride, const uint64_t* tau_g2_aff,
                                       const uint64_t* points, int32_t point_mode, const uint64_t* values, const uint64_t* proofs_aff, size_t n,
                                       uint8_t* status, uint64_t* n_bad, uint64_t* first_bad, uint64_t* lhs_out_aff);
keaki_status keaki_hip_kzg_verify_each_dev(keaki_hip_ctx* ctx, const void* d_com_aff, int32_t com_stride, const void* d_tau_g2_aff,
                                           const void* d_points, int32_t point_mode, const void* d_values, const void* d_proofs_aff, size_t n,
                                           void* d_status, uint64_t* n_bad, uint64_t* first_bad, void* d_lhs_out_aff);

/* ---- SRS ingest (scope row f-3) -----------------------------------------------------------------------------------------
 * The reference reads .ptau points with `deserialize_uncompressed_unchecked` (src/kzg/ptau.rs:266,314): no curve check at all.
 * A snarkjs .ptau stores coordinates as Montgomery limbs, which is this ABI's point layout, so sections 2 and 3 are uploaded
 * verbatim (keaki_hip_srs_g1_upload) and checked on the device: the number of points with y^2 != x^3 + b (b = 3 on G1,
 * 3/(9+u) on the twist; (0,0) = identity passes) and the index of the first one (UINT64_MAX if none; may be NULL). */
keaki_status keaki_hip_srs_g1_check(keaki_hip_ctx* ctx, const keaki_hip_srs_g1* srs, uint64_t* n_off_curve, uint64_t* first_off_curve);
keaki_status keaki_hip_g2_check(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint64_t* n_off_curve, uint64_t* first_off_curve);

/* ---- compressed point wire format: what crosses a trust boundary -----------------------------------------------------------
 * The byte format of ark-serialize 0.4.2 `serialize_compressed` for short-Weierstrass affine points (restated from memory, not pinned
 * against a Rust build: DESIGN section 2), half the size of the limb layout:
 *   G1, 32 bytes   x as a canonical (non-Montgomery) little-endian integer; p has 254 bits, so bits 6 and 7 of byte 31 are free
 *   G2, 64 bytes   x.c0 then x.c1, 32 B little-endian each; the flags sit in byte 63
 *   flags          bit 7 = YIsNegative, set iff y > -y (Fq: on canonical integers; Fq2: c1 is compared first, c0 when the c1 are equal);
 *                  bit 6 = PointAtInfinity; the identity encodes as x = 0 with bit 6 set
 * compress: n affine points in this ABI's Montgomery limb layout ((0,0) = identity) -> n x 32 B / n x 64 B. The points are taken as they
 * are: an input that is not on the curve produces bytes that decompress rejects or decodes to another point.
 * decompress -- the decoding rule of this library. An item is REJECTED when
 *   status 1 (malformed)   both flag bits are set, x (or a coordinate of x) is >= p, or the identity flag comes with x != 0
 *   status 2               x^3 + b is not a square (b = 3 on G1, 3/(9+u) on the twist): no point of the curve has this x
 *   status 3               G2 with check_subgroup = 1: the point lies on the twist but outside the subgroup of order r. BN254's twist has a
 *                          cofactor 2p - r of about 2^254, so a G2 point from another party MUST be checked before it is paired
 *                          (arkworks' `deserialize_compressed` validates by default). G1 has cofactor 1: on the curve is in the group.
 * otherwise (status 0) y is the root the sign flag names. out_aff: n affine points in the limb layout, a rejected item all zero.
 * status: uint8_t[n] or NULL. n_bad: the number of rejected items (required); first_bad: the index of the first one, UINT64_MAX if none
 * (may be NULL) -- shaped like keaki_hip_g2_check. One bad item does not fail the call: the return value stays KEAKI_OK.
 * check_subgroup outside {0, 1}, a null bytes / out_aff / n_bad pointer with n > 0: KEAKI_ERR_BAD_ARG. n = 0: *n_bad = 0.
 * keaki_hip_g2_subgroup_check: the same membership test for callers that already hold uncompressed points (it complements keaki_hip_g2_check,
 * which tests the curve equation only; the points are assumed to be on the twist). n_outside / first_outside as above; the identity passes.
 * The test is psi(Q) = [6 z^2]Q (psi: untwist-Frobenius-twist), which holds exactly on the subgroup.
 * Host forms go through the stager of the KEM host batches; from 65,536 items on they run as its chunk pipeline (two halves, then chunks
 * of 65,536: upload, kernels and download overlap; option "pipe_chunks" = 0: one chunk) and return when the results are in place. _dev: bytes, points and status are device pointers; the counters stay HOST pointers,
 * so these forms synchronise as well. Device buffers must be 16-byte aligned. n < 2^31 per call. */
keaki_status keaki_hip_g1_compress(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint8_t* bytes_out);
keaki_status keaki_hip_g2_compress(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint8_t* bytes_out);
keaki_status keaki_hip_g1_compress_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, void* d_bytes_out);
keaki_status keaki_hip_g2_compress_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, void* d_bytes_out);
keaki_status keaki_hip_g1_decompress(keaki_hip_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* out_aff, uint8_t* status, uint64_t* n_bad,
                                     uint64_t* first_bad);
keaki_status keaki_hip_g2_decompress(keaki_hip_ctx* ctx, const uint8_t* bytes, size_t n, int32_t check_subgroup, uint64_t* out_aff, uint8_t* status,
                                     uint64_t* n_bad, uint64_t* first_bad);
keaki_status keaki_hip_g1_decompress_dev(keaki_hip_ctx* ctx, const void* d_bytes, size_t n, void* d_out_aff, void* d_status, uint64_t* n_bad,
                                         uint64_t* first_bad);
keaki_status keaki_hip_g2_decompress_dev(keaki_hip_ctx* ctx, const void* d_bytes, size_t n, int32_t check_subgroup, void* d_out_aff, void* d_status,
                                         uint64_t* n_bad, uint64_t* first_bad);
keaki_status keaki_hip_g2_subgroup_check(keaki_hip_ctx* ctx, const uint64_t* points_aff, size_t n, uint64_t* n_outside, uint64_t* first_outside);
keaki_status keaki_hip_g2_subgroup_check_dev(keaki_hip_ctx* ctx, const void* d_points_aff, size_t n, uint64_t* n_outside, uint64_t* first_outside);

/* ---- batched scalar multiplication: replaces `.mul(scalar)` (src/kem.rs:22,30,36,37; src/kzg.rs:57,60,135,144)
 * out[i] = scalars[i] * points[i]   (point_stride = 1) or scalars[i] * points[0] (point_stride = 0).
 * points affine in, affine out. */
keaki_status keaki_hip_g1_mul_batch(keaki_hip_ctx* ctx, const uint64_t* points_aff, int32_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_aff);
keaki_status keaki_hip_g2_mul_batch(keaki_hip_ctx* ctx, const uint64_t* points_aff, int32_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_aff);
keaki_status keaki_hip_g1_mul_batch_dev(keaki_hip_ctx* ctx, const void* d_points_aff, int32_t point_stride, const void* d_scalars, size_t n, void* d_out_aff);
keaki_status keaki_hip_g2_mul_batch_dev(keaki_hip_ctx* ctx, const void* d_points_aff, int32_t point_stride, const void* d_scalars, size_t n, void* d_out_aff);

/* ---- batched pairing: replaces E::pairing(p, q) (src/kem.rs:30,58; src/kzg.rs:148) + serialize_uncompressed (src/kem.rs:32,61)
 * gt_out[i] = serialize_uncompressed(e(g1[i], g2[i * g2_stride])); identity in either slot -> GT one. */
keaki_status keaki_hip_pairing_batch(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, int32_t g2_stride, size_t n, uint8_t* gt_out);
keaki_status keaki_hip_pairing_batch_dev(keaki_hip_ctx* ctx, const void* d_g1_aff, const void* d_g2_aff, int32_t g2_stride, size_t n, void* d_gt_out);

/* ---- KEM composites: the bodies of the loops at src/vec.rs:63-66 and :75-78 --------------------
 * encap_batch: for i < n (src/kem.rs:13-50 with the SAME com / tau_g2 for all i):
 *     ct[i]  = r[i] * (tau_g2 - points[i] * g2)                       (affine G2, u64[16])
 *     gt[i]  = serialize(e(r[i] * (com - values[i] * g1), g2))        (384 bytes)
 *     key[i] = BLAKE3-XOF(gt[i])[0..msg_len]   if key_out != NULL     (src/kem.rs:42-46)
 * r[i] are drawn by the caller (one Fr::rand per item in index order, src/kem.rs:26) so the
 * randomness stream is the caller's. gt_out may be NULL when only keys are wanted. msg_len <= 1<<16.
 * The host-array forms (no _dev suffix) of encap / decap / encrypt / decrypt_batch run batches of two chunks or more (2^16 items; the
 * pairing side: 2^17) as a pipeline -- uploads and downloads on a stream of the context's own under the neighbouring chunks' kernels --
 * and first-touch the caller's output pages from up to three short-lived helper threads ahead of the downloads (a download into pages
 * that do not exist yet runs at a tenth of the link rate). Results are those of one call per chunk; the call returns when every byte
 * has been delivered and every helper has been joined. An output array may be one of the input arrays (messages in, bodies out): a chunk's
 * output pages are touched only after its inputs have been read; arrays the HIP runtime knows (hipHostMalloc / hipHostRegister) are not touched. */
keaki_status keaki_hip_encap_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff,
                                   const uint64_t* points, const uint64_t* values, const uint64_t* r, size_t n,
                                   uint64_t* ct_out_aff, uint8_t* gt_out, uint8_t* key_out, size_t msg_len);
keaki_status keaki_hip_encap_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_tau_g2_aff,
                                       const void* d_points, const void* d_values, const void* d_r, size_t n,
                                       void* d_ct_out_aff, void* d_gt_out, void* d_key_out, size_t msg_len);
/* Setup-time (optional): everything of encap_batch that depends on the SETUP only -- the fixed-base window tables of g1, g2 and [tau]_2, the
 * line sequence of g2 and, for batch_hint >= 65,536, the GT table of e(g1, g2) -- built now instead of inside the first large encap_batch of
 * the context (~60 ms). The KEM analogue of keaki_hip_srs_g1_precompute; results never depend on it. */
keaki_status keaki_hip_encap_prepare(keaki_hip_ctx* ctx, const uint64_t* tau_g2_aff, size_t batch_hint);
/* decap_batch (src/kem.rs:55-72): gt[i] = serialize(e(proofs[i], cts[i])), key[i] = BLAKE3-XOF(gt[i]) */
keaki_status keaki_hip_decap_batch(keaki_hip_ctx* ctx, const uint64_t* proofs_aff, const uint64_t* cts_aff, size_t n,
                                   uint8_t* gt_out, uint8_t* key_out, size_t msg_len);
keaki_status keaki_hip_decap_batch_dev(keaki_hip_ctx* ctx, const void* d_proofs_aff, const void* d_cts_aff, size_t n,
                                       void* d_gt_out, void* d_key_out, size_t msg_len);

/* ---- enc::encrypt / enc::decrypt over a batch: KEM + the XOR DEM on the device ---------------------------------------------
 * Replaces the body of the loops of vec_encrypt / vec_decrypt (src/vec.rs:63-66, :75-78), i.e. src/enc.rs:19-40 and :44-55 per item:
 * encapsulate / decapsulate as above, then `key XOR message` (src/enc.rs:32-36, :48-52) inside the KDF kernel -- neither the 384 GT bytes nor
 * the key leave the device. n messages of msg_len (1..65536) bytes each, contiguous. r[i] drawn by the caller as for encap_batch.
 * _dev: d_body_inout holds the messages on entry and the ciphertext bodies on exit (decrypt: bodies in, messages out). */
keaki_status keaki_hip_encrypt_batch(keaki_hip_ctx* ctx, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* points,
                                     const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n, uint64_t* ct_out_aff,
                                     uint8_t* body_out, size_t msg_len);
keaki_status keaki_hip_encrypt_batch_dev(keaki_hip_ctx* ctx, const void* d_com_aff, const void* d_tau_g2_aff, const void* d_points,
                                         const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff, void* d_body_inout, size_t msg_len);
keaki_status keaki_hip_decrypt_batch(keaki_hip_ctx* ctx, const uint64_t* proofs_aff, const uint64_t* cts_aff, const uint8_t* bodies, size_t n,
                                     uint8_t* msgs_out, size_t msg_len);
keaki_status keaki_hip_decrypt_batch_dev(keaki_hip_ctx* ctx, const void* d_proofs_aff, const void* d_cts_aff, size_t n, void* d_body_inout,
                                         size_t msg_len);

/* ---- encap_multi / encrypt_multi: encapsulate and encrypt to MANY commitments in one call -------------------------------------------------
 * The sender of a many-party flow answers m receivers, each with its own commitment (vec_encrypt, src/vec.rs:52-69, once per receiver). One
 * call replaces m calls of encap_batch / encrypt_batch, each of which pays the launch floor and, for a commitment seen for the first time, a
 * GT table of e(C, g2) (1.7 ms, 31.5 MB).
 * Layout: coms_aff = m affine G1 points (u64[8] each, (0,0) = the identity); offsets = uint64_t[m + 1], group j = items
 *   [offsets[j], offsets[j + 1]), empty groups allowed anywhere; every other array item-major as in encap_batch / encrypt_batch.
 *   r[i] drawn by the caller, one per item in GLOBAL index order: the stream that m consecutive vec_encrypt calls draw.
 * Results: for every group j the ct, gt, key and body bytes of its items are byte for byte those of keaki_hip_encap_batch /
 *   keaki_hip_encrypt_batch for (coms[j], the group's items) alone -- whichever route the group takes, with long or small tables.
 * Routes: a group of at least "encap_multi_single_min" items (keaki_hip_ctx_set_option; 0 = never) runs the single-commitment path on its
 *   item range (GT tables: worth their build from some thousand items on). Every other item runs the FUSED route, in maximal runs of
 *   consecutive small groups: the ciphertext kernel of encap_batch, one G1 kernel that finds each item's commitment in `offsets` and computes
 *   r_i C_j + (-(r_i beta_i)) g1 with one inversion, a pairing per item against g2's tabulated lines, the KDF. It builds no table per
 *   commitment and leaves the single-commitment path's cache (its GT table, its count of repeated commitments) alone.
 *   The default of "encap_multi_single_min", 16,384, is MEASURED (profiles/encap_multi_times.txt, written by bench_tools/bench_encap_multi.py):
 *   with 16 groups of k items the fused route wins at k = 1,024 and 4,096 (0.75 against 2.2 ms per group at 4,096) and the single route at
 *   16,384 and 65,536 (2.05 against 2.95 ms per group at 16,384); no k between 4,096 and 16,384 was measured. The estimate before the sweep
 *   (a 1.7 ms table, partly overlapped, against ~0.13 us saved per item) was 8,192.
 * Errors: KEAKI_ERR_BAD_ARG with nothing written for a null pointer (gt_out or key_out may be NULL, not both, as in encap_batch),
 *   offsets[0] != 0, a decreasing offset, offsets[m] != n, n >= 2^31, m >= 2^31, msg_len > 65536 (encrypt: also msg_len == 0). n == 0
 *   (m == 0 included) writes nothing and returns KEAKI_OK.
 * Host form: one fused run is one pipelined batch (chunks of 2^15 items from 2^16 items on; a chunk may begin inside a group); a large group
 *   is the host form of encap_batch / encrypt_batch on its sub-range of the caller's arrays. A failing call returns only when nothing reads
 *   or writes caller memory any more.
 * _dev: `offsets` is a HOST pointer here too, read before the call returns (as the domain constants of open_fk_poly_batch_dev). The call
 *   synchronises where encap_batch_dev does -- the one read-back of [tau]_2 that keys its table -- and reads back a commitment only for a
 *   group that takes the single-commitment route. d_body_inout: messages in, bodies out, in place.
 * Context: one context, one device; sharding over a device group is not offered. */
keaki_status keaki_hip_encap_multi(keaki_hip_ctx* ctx, const uint64_t* coms_aff, const uint64_t* offsets, size_t m, const uint64_t* tau_g2_aff,
                                   const uint64_t* points, const uint64_t* values, const uint64_t* r, size_t n, uint64_t* ct_out_aff,
                                   uint8_t* gt_out, uint8_t* key_out, size_t msg_len);
keaki_status keaki_hip_encap_multi_dev(keaki_hip_ctx* ctx, const void* d_coms_aff, const uint64_t* offsets, size_t m, const void* d_tau_g2_aff,
                                       const void* d_points, const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff,
                                       void* d_gt_out, void* d_key_out, size_t msg_len);
keaki_status keaki_hip_encrypt_multi(keaki_hip_ctx* ctx, const uint64_t* coms_aff, const uint64_t* offsets, size_t m, const uint64_t* tau_g2_aff,
                                     const uint64_t* points, const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n,
                                     uint64_t* ct_out_aff, uint8_t* body_out, size_t msg_len);
keaki_status keaki_hip_encrypt_multi_dev(keaki_hip_ctx* ctx, const void* d_coms_aff, const uint64_t* offsets, size_t m, const void* d_tau_g2_aff,
                                         const void* d_points, const void* d_values, const void* d_r, size_t n, void* d_ct_out_aff,
                                         void* d_body_inout, size_t msg_len);

/* ---- device group: in-process multi-GPU (SURVEY 8b `_create(n_devices)`, 8e "single process, one host thread per GPU") -----------------
 * What a Rust caller of keaki gets with more than one GPU and no PyTorch / RCCL: the library keeps one ctx and one host worker thread per
 * entry of `devices` (an ordinal may repeat: several contexts on one GPU, which is how the single-GPU test box exercises it), the SRS is
 * split into contiguous chunks, chunk i resident on devices[i] with ITS window tables (built in parallel at upload), and
 *   keaki_hip_group_msm_g1      = commit's MSM (src/kzg.rs:98): every member runs a complete Pippenger on its (scalar, point) range, the
 *                                 N partial sums (96 B each) come back through host memory -- no collective in-process -- and member 0
 *                                 adds them (keaki_hip_g1_sum). EC addition is exact: the affine result equals the one-GPU result.
 *   keaki_hip_group_kzg_open    = `open` (src/kzg.rs:104-124): quotient on member 0, then the group MSM.
 *   keaki_hip_group_encap_batch / _decap_batch = the loops of vec_encrypt / vec_decrypt (src/vec.rs:63-66, :75-78) split by item range,
 *                                 every member writing straight into its slice of the caller's output arrays.
 * Ranges follow the SRS (member i owns points [i*len/N ...)), not the polynomial, so the tables serve every polynomial.
 * Errors: the first failing member's status; keaki_hip_group_last_error names the member. Calls on one group are serialised. */
typedef struct keaki_hip_group keaki_hip_group;
typedef struct keaki_hip_group_srs_g1 keaki_hip_group_srs_g1;
keaki_status keaki_hip_group_create(const int32_t* devices, size_t n_devices, keaki_hip_group** out);
void keaki_hip_group_destroy(keaki_hip_group* g);
size_t keaki_hip_group_size(const keaki_hip_group* g);
keaki_hip_ctx* keaki_hip_group_ctx(const keaki_hip_group* g, size_t member);   /* member's ctx, e.g. for verify / open_fk on member 0 */
const char* keaki_hip_group_last_error(const keaki_hip_group* g);               /* g may be NULL: last create error */
/* keaki_hip_group_create enables peer access between every pair of distinct devices (the exchanges of the sharded FK23 are then device-to-device
 * copies on the members' streams, ordered by events). "" when every pair has it; otherwise the pairs whose copies the runtime stages. */
const char* keaki_hip_group_peer_note(const keaki_hip_group* g);
/* precompute != 0: also build every chunk's window tables (KEAKI_ERR_OOM of a table is tolerated: that member runs the generic MSM) */
keaki_status keaki_hip_group_srs_g1_upload(keaki_hip_group* g, const uint64_t* points_aff, size_t n, int32_t precompute, keaki_hip_group_srs_g1** out);
size_t keaki_hip_group_srs_g1_len(const keaki_hip_group_srs_g1* srs);
int32_t keaki_hip_group_srs_g1_has_tables(const keaki_hip_group_srs_g1* srs);  /* 1: every member that holds points holds their window tables */
void keaki_hip_group_srs_g1_free(keaki_hip_group* g, keaki_hip_group_srs_g1* srs);
keaki_status keaki_hip_group_msm_g1(keaki_hip_group* g, const keaki_hip_group_srs_g1* srs, const uint64_t* scalars, size_t n, uint64_t* out_jac);
keaki_status keaki_hip_group_kzg_open(keaki_hip_group* g, const keaki_hip_group_srs_g1* srs, const uint64_t* coeffs, size_t n, const uint64_t* point,
                                      uint64_t* proof_out_jac, uint64_t* value_out);
keaki_status keaki_hip_group_encap_batch(keaki_hip_group* g, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* points,
                                         const uint64_t* values, const uint64_t* r, size_t n, uint64_t* ct_out_aff, uint8_t* gt_out,
                                         uint8_t* key_out, size_t msg_len);
keaki_status keaki_hip_group_decap_batch(keaki_hip_group* g, const uint64_t* proofs_aff, const uint64_t* cts_aff, size_t n, uint8_t* gt_out,
                                         uint8_t* key_out, size_t msg_len);
/* the same split for keaki_hip_encrypt_batch / keaki_hip_decrypt_batch (KEM + XOR DEM on the members) */
keaki_status keaki_hip_group_encrypt_batch(keaki_hip_group* g, const uint64_t* com_aff, const uint64_t* tau_g2_aff, const uint64_t* points,
                                           const uint64_t* values, const uint64_t* r, const uint8_t* msgs, size_t n, uint64_t* ct_out_aff,
                                           uint8_t* body_out, size_t msg_len);
keaki_status keaki_hip_group_decrypt_batch(keaki_hip_group* g, const uint64_t* proofs_aff, const uint64_t* cts_aff, const uint8_t* bodies, size_t n,
                                           uint8_t* msgs_out, size_t msg_len);

/* kzg::open_fk (src/kzg.rs:157-203) over the members of a group: the sharded FK23 pipeline (keaki_hip_fk_shard_*, member i = rank i) with the
 * exchanges done inside the library -- device-to-device copies between the members' buffers (hipMemcpyPeer), no collective, no RCCL. The
 * handle keeps srs[0..d) on every member (points_aff: the first d = 2^log2d points of the SRS) and every member's part of the SRS-only
 * transform. Needs a power-of-two group and d >= N^2; any other shape runs un-sharded on member 0. omega_2d, omega_2d_inv, inv_2d as for
 * keaki_hip_open_fk_poly. _open: coeffs = d Fr on the host, proofs_out_aff = d affine points, the bytes keaki_hip_open_fk_poly returns. */
typedef struct keaki_hip_group_fk keaki_hip_group_fk;
keaki_status keaki_hip_group_fk_create(keaki_hip_group* g, const uint64_t* points_aff, uint32_t log2d, const uint64_t* omega_2d,
                                       const uint64_t* omega_2d_inv, const uint64_t* inv_2d, keaki_hip_group_fk** out);
keaki_status keaki_hip_group_fk_open(keaki_hip_group* g, keaki_hip_group_fk* fk, const uint64_t* coeffs, uint64_t* proofs_out_aff);
void keaki_hip_group_fk_free(keaki_hip_group* g, keaki_hip_group_fk* fk);

/* ---- instrumentation (bench.py reads these; not part of the reference surface) ---------------- */
/* device time in milliseconds of the dominant kernel (bucket accumulation) of the last msm_*_dev
 * call, measured with HIP events on the ctx stream; < 0 if timing is disabled. */
keaki_status keaki_hip_set_timing(keaki_hip_ctx* ctx, int32_t enabled);
float keaki_hip_last_msm_bucket_ms(const keaki_hip_ctx* ctx);
float keaki_hip_last_msm_total_ms(const keaki_hip_ctx* ctx);
/* device time (ms) of the last keaki_hip_open_fk[_poly] call made while timing was enabled: out3 = [the 2d pointwise scalar-mults, the butterfly
 * stages of the two size-d group transforms (the dominant kernel k_g1_fft_stage_map), the whole device pipeline]; < 0 when there was none */
keaki_status keaki_hip_last_fk_ms(keaki_hip_ctx* ctx, float* out3);
/* window size (bits) the last MSM used. An MSM over n = 0 terms uses none and measures nothing: after it, this and the two times above are
 * still those of the last non-empty MSM (also when that one was still queued in front of the empty call). */
int32_t keaki_hip_last_msm_window_bits(const keaki_hip_ctx* ctx);

/* Test hook: final exponentiation alone. f_mont: n x 12 Fq (Montgomery limbs, order c0.c0.c0 ... c1.c2.c1), the output of a
 * Miller loop; gt_out: n x 384 bytes, as keaki_hip_pairing_batch would emit. Lets the tests bisect Miller loop vs final exponent. */
keaki_status keaki_hip_g2_prepare(keaki_hip_ctx* ctx, const uint64_t* g2_aff, uint64_t* lines_out, size_t lines_out_bytes);
keaki_status keaki_hip_miller_loop_batch(keaki_hip_ctx* ctx, const uint64_t* g1_aff, const uint64_t* g2_aff, size_t n, uint64_t* f_mont_out);
keaki_status keaki_hip_final_exp_batch(keaki_hip_ctx* ctx, const uint64_t* f_mont, size_t n, uint8_t* gt_out);

/* On-device self-test: runs the hand-scheduled Fq instruction streams (product, add, sub, neg, square and a
 * dependent chain) against the portable template code on `blocks` x 256 lanes x `iters` random and corner-case
 * inputs; *mismatches_out must come back 0. */
keaki_status keaki_hip_selftest_field(keaki_hip_ctx* ctx, uint32_t blocks, uint32_t iters, uint32_t seed, uint64_t* mismatches_out);

/* Field probe: ONE shipped field function on operands the HOST chose, raw result limbs back (tests/test_gpu_field_ops.py compares them
 * with Python integers, exactly). Record layout:
 *   operands: n records of 12 slots x 9 uint32_t. A lazy operand (9 x 29-bit limbs, any u32 per limb) fills its slot; a saturated operand
 *             (8 x 32-bit words) uses words 0..7 of its slot. Operand k of an op is slot k; unused slots are ignored.
 *   out:      n records of 9 uint32_t: the raw result. Saturated results use words 0..7, predicates word 0 (0 / 1); the rest is 0.
 * One record per lane, 64 lanes per workgroup. The lane-pair ops (KEAKI_FOP_FQ2_MUL and above) take records 2r and 2r + 1 as the c0 and c1
 * lanes of one Fq2 element: n must be even (the library pads the launch to whole waves with copies of record 0; only the first n records
 * are stored). 1 <= n <= 65536; an unknown op, n out of range, an odd n of a lane-pair op or a null pointer is KEAKI_ERR_BAD_ARG and
 * launches nothing. KEAKI_FOP_FQ_INV_XGCD answers a non-canonical operand (>= p) with all-ones words instead of running (its loop would
 * not end). Operand bounds are the callee's own (fq29_core.hip.h, fq29_asm.hip.h, pair261.hip.h); the probe does not check them. */
#define KEAKI_FOP_FIRST_PAIR KEAKI_FOP_FQ2_MUL
#define KEAKI_FOP_SLOTS 12
#define KEAKI_FOP_SLOT_WORDS 9
#define KEAKI_FOP_MAX_RECORDS 65536
typedef enum {
  /* 9 x 29-bit lazy streams (fq29_core.hip.h, fq29_asm.hip.h, fq29_dot_asm.hip.h) */
  KEAKI_FOP_U29_MUL = 0,             /* u29_mul(s0, s1): s0 is the wide side */
  KEAKI_FOP_U29_MUL_REF = 1,
  KEAKI_FOP_U29_SQR = 2,
  KEAKI_FOP_U29_SQR_REF = 3,
  KEAKI_FOP_U29_MUL2 = 4,            /* u29_mul2(s0, s1, s2, s3) = s0 s1 + s2 s3 */
  KEAKI_FOP_U29_DOT3 = 5,            /* sum of s(2k) s(2k+1), k < 3 */
  KEAKI_FOP_U29_DOT4 = 6,
  KEAKI_FOP_U29_DOT6 = 7,
  KEAKI_FOP_U29_CARRY = 8,
  KEAKI_FOP_U29_SUB_K2 = 9,          /* u29_sub(s0, s1, Q29::K2) ... */
  KEAKI_FOP_U29_SUB_K4 = 10,
  KEAKI_FOP_U29_SUB_K4W = 11,
  KEAKI_FOP_U29_SUB_K8 = 12,
  KEAKI_FOP_U29_SUB_K16 = 13,
  KEAKI_FOP_U29_SUB_K16W = 14,
  KEAKI_FOP_U29_SUB_K32 = 15,
  KEAKI_FOP_U29_SUB_K64 = 16,
  KEAKI_FOP_U29_SUB_K128 = 17,
  KEAKI_FOP_U29_SUB_RAW_K16 = 18,    /* u29_sub_raw(s0, s1, K) */
  KEAKI_FOP_U29_SUB_RAW_K32 = 19,
  KEAKI_FOP_U29_SUB3 = 20,           /* u29_sub3(s0, s1, s2) */
  KEAKI_FOP_U29_MAYBE_ZERO = 21,
  KEAKI_FOP_U29_MAYBE_ZERO34 = 22,
  KEAKI_FOP_U29_IS_ZERO = 23,
  KEAKI_FOP_U29_PACK_CANONICAL = 24, /* limbs -> 8 words */
  KEAKI_FOP_U29_FROM_SAT_SHIFT5 = 25,/* 8 words -> limbs */
  KEAKI_FOP_U29_FROM_SAT_PLAIN = 26,
  KEAKI_FOP_U29_FROM_FQ = 27,
  KEAKI_FOP_U29_TO_FQ = 28,
  KEAKI_FOP_U29_TO_SAT = 29,
  /* saturated 8 x 32 streams (bn254_field.hip.h, bn254_field_asm.hip.h), Montgomery radix 2^256 */
  KEAKI_FOP_FQ_MUL = 30,
  KEAKI_FOP_FQ_SQR = 31,
  KEAKI_FOP_FQ_ADD = 32,
  KEAKI_FOP_FQ_SUB = 33,
  KEAKI_FOP_FQ_NEG = 34,
  KEAKI_FOP_FQ_DBL = 35,
  KEAKI_FOP_FQ_HALF = 36,
  KEAKI_FOP_FQ_REDUCE_ONCE = 37,     /* fp_reduce_once<FqParamsRef> */
  KEAKI_FOP_FQ_INV_XGCD = 38,
  KEAKI_FOP_FQ_INV_SAFEGCD = 39,
  KEAKI_FOP_FQ_INV_FERMAT = 40,
  KEAKI_FOP_FQ_INV = 41,             /* fq_inv: the inverse the kernels call */
  KEAKI_FOP_FR_FROM_MONT = 42,       /* fp_from_mont<FrParams> */
  KEAKI_FOP_FR_MUL = 43,
  KEAKI_FOP_FR_ADD = 44,
  KEAKI_FOP_FR_SUB = 45,
  /* 2^261 form of the pairing tower (pair261.hip.h), one lane per record */
  KEAKI_FOP_TO261 = 46,
  KEAKI_FOP_TO256 = 47,
  KEAKI_FOP_CANON_WORDS = 48,
  KEAKI_FOP_FQ_INV261 = 49,
  /* lane-pair ops: every op from here on */
  KEAKI_FOP_FQ2_MUL = 50,
  KEAKI_FOP_FQ2_SQR = 51,
  KEAKI_FOP_FQ2_MUL_XI = 52,
  KEAKI_FOP_FQ2_MUL_FQ = 53,         /* s1: this lane's Fq factor */
  KEAKI_FOP_FQ2_INV = 54,
  KEAKI_FOP_FQ2_CONJ = 55,
  KEAKI_FOP_FQ2_NEG = 56,
  KEAKI_FOP_FQ4_SQR_T0 = 57,         /* fq4_sqr(&t0, &t1, s0, s1) */
  KEAKI_FOP_FQ4_SQR_T1 = 58,
  KEAKI_FOP_FQ6_MUL_C0 = 59,         /* fq6_mul of (s0, s1, s2) by (s3, s4, s5) */
  KEAKI_FOP_FQ6_MUL_C1 = 60,
  KEAKI_FOP_FQ6_MUL_C2 = 61,
  KEAKI_FOP_COUNT = 62
} keaki_field_op;
keaki_status keaki_hip_selftest_field_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out);

/* Tower probe: ONE shipped function of the pairing's Fq12 tower (pair261.hip.h, pairing.hip.h) or of its twelve-lane form
 * (pairing_wide.hip.h) on operands the HOST chose, all twelve result words back (tests/test_gpu_tower_ops.py compares them with Python
 * integers, exactly). The field probe above stops at fq6_mul; this one starts there. Record layout (uint32_t words):
 *   operands: n records of KEAKI_TOP_REC_WORDS words
 *     A    [  0,  96)  Fq12 operand a: 12 Fq in the tower's memory order c0.c0.c0, c0.c0.c1, c0.c1.c0 ... c1.c2.c1 (Fq2 coefficient m = 3 h + j
 *                      of c_h.c_j, component e at Fq index 2 m + e), 8 canonical words each (< p), residue x 2^261 mod p
 *     B    [ 96, 192)  Fq12 operand b, the same form
 *     LINE [192, 246)  a line c0 + (d0 + d1 v) w as LIMBS: c0.c0, c0.c1, d0.c0, d0.c1, d1.c0, d1.c1, nine 29-bit limbs each; exact limbs,
 *                      value < 2p (c0, d0) | < p (d1), what fq12_mul_by_034_limbs and w12_mul_034 take
 *     T    [246, 294)  running point (X, Y, Z), homogeneous projective on the twist: 3 Fq2 = 6 Fq of 8 canonical words (2^261 form).
 *                      KEAKI_TOP_ELL reads its Line (c0, c1, c2 as Fq2 words) here
 *     Q    [294, 326)  affine point (x, y): 2 Fq2 = 4 Fq of 8 canonical words
 *     P    [326, 344)  P.x, P.y as nine exact limbs each, value < p (KEAKI_TOP_ELL)
 *   out:      n records of KEAKI_TOP_OUT_WORDS words: 12 Fq of 8 canonical words, 2^261 form. Fq12 results in the tower's memory order;
 *             the line functions give T' = (X, Y, Z) in Fq 0..5 and the line (c0, c1, c2) in Fq 6..11; KEAKI_TOP_FQ6_INV inverts c0 of A
 *             into Fq 0..5 and leaves 6..11 zero. An op reads the areas its function takes and ignores the rest.
 * Geometry. Lane-pair ops (below KEAKI_TOP_FIRST_WIDE): one record per lane pair, 32 per wave, the even lane holds component 0; 18 Fq of LDS
 * parking per lane as k_pairing. Wide ops: one record per 16-lane row, 4 per wave; lane pair k of a row holds the flat coefficient of w^k
 * (k = 2 j + e for c_e.c_j), lanes 12..15 shadow pairs 0 and 1 and store nothing; the exchange area is k_pairing_wide's. The wide line
 * functions keep T in every pair: pair k stores Fq2 number k of the six results. All 64 lanes run: the library pads the launch to whole waves
 * with copies of record 0 and only the first n records are stored. 1 <= n <= KEAKI_TOP_MAX_RECORDS; an unknown op, n out of range or a
 * null pointer is KEAKI_ERR_BAD_ARG and launches nothing. Operand bounds are the callee's own; the probe does not check them.
 * Every op is one call with the template arguments of a shipped call site (k_pairing, k_pairing2, k_gt_table_fill, k_gt_encap_exp,
 * k_pairing_wide and its kin). Not probed: fq12_sqr<false>, fq12_cyc_sqr<false> and fq12_mul_by_034_limbs<false> (only the on-device
 * self-test instantiates them); w12_mul_forms apart from line_forms (w12_mul_034 is exactly that pair of calls); the addition operand of the
 * st = 3, 4, 5 Miller steps (Fq2 ops of the field probe, applied before the call); the two-wave choreography of k_pairing_wide2 (its
 * functions are the ones probed here, its scheduling stays with the end-to-end tests); the GT window tables (tests/test_gpu_fb_digit_edges.py). */
#define KEAKI_TOP_REC_WORDS 344
#define KEAKI_TOP_OUT_WORDS 96
#define KEAKI_TOP_MAX_RECORDS 4096
#define KEAKI_TOP_FIRST_WIDE KEAKI_TOP_W12_MUL
typedef enum {
  /* lane-pair form (pair261.hip.h, pairing.hip.h) */
  KEAKI_TOP_FQ12_MUL = 0,            /* fq12_mul(&a, &a, &b) */
  KEAKI_TOP_FQ12_MUL_LD = 1,         /* fq12_mul_ld<true>(&a, &a, halves of B from memory, park) */
  KEAKI_TOP_FQ12_SQR = 2,            /* fq12_sqr<true>(&a, &a, park, 3) */
  KEAKI_TOP_FQ12_INV = 3,            /* fq12_inv<false>: 0 -> 0 */
  KEAKI_TOP_FQ12_INV_PARKED = 4,     /* fq12_inv<true>(&a, &a, park) */
  KEAKI_TOP_FQ12_CONJ = 5,
  KEAKI_TOP_FQ12_CYC_SQR = 6,        /* fq12_cyc_sqr<true>(&a, &a, park): total, the square on unitary elements */
  KEAKI_TOP_FQ12_FROB1 = 7,          /* fq12_frob(&a, &a, k), k = 1, 2, 3 (k is a run-time value, as in the kernels) */
  KEAKI_TOP_FQ12_FROB2 = 8,
  KEAKI_TOP_FQ12_FROB3 = 9,
  KEAKI_TOP_FQ12_FROB_PARKED1 = 10,  /* fq12_frob_parked(&a, &a, k, park) */
  KEAKI_TOP_FQ12_FROB_PARKED2 = 11,
  KEAKI_TOP_FQ12_FROB_PARKED3 = 12,
  KEAKI_TOP_FQ12_MUL_BY_034 = 13,    /* fq12_mul_by_034_limbs<true>(&a, c0, d0, d1, true, park, 3) on LINE */
  KEAKI_TOP_ELL = 14,                /* ell(&a, line words in T, P.x, P.y, park, 3) */
  KEAKI_TOP_FQ6_INV = 15,            /* fq6_inv of a.c0: 0 -> 0 */
  KEAKI_TOP_LINE_DOUBLE = 16,        /* line_double(&T, &l) */
  KEAKI_TOP_LINE_ADD = 17,           /* line_add(&T, &Q.x, &Q.y, &l) */
  /* twelve-lane form (pairing_wide.hip.h): every op from here on */
  KEAKI_TOP_W12_MUL = 18,
  KEAKI_TOP_W12_MUL_034 = 19,        /* w12_mul_034 = w12_mul_forms(a, line_forms(c0, d0, d1)) on LINE */
  KEAKI_TOP_W12_CYC_SQR = 20,
  KEAKI_TOP_W12_FROB1 = 21,
  KEAKI_TOP_W12_FROB2 = 22,
  KEAKI_TOP_W12_FROB3 = 23,
  KEAKI_TOP_W12_CONJ = 24,
  KEAKI_TOP_W12_INV = 25,            /* w12_gather, fq12_inv<false>, w12_own */
  KEAKI_TOP_W12_GATHER_OWN = 26,     /* w12_own(w12_gather(a)): the element itself */
  KEAKI_TOP_W_LINE_DOUBLE = 27,
  KEAKI_TOP_W_LINE_ADD = 28,
  KEAKI_TOP_COUNT = 29
} keaki_tower_op;
keaki_status keaki_hip_selftest_tower_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out);

/* Point probe: ONE shipped function of the group law in the 9 x 29-bit lazy limbs (xyzz29.hip.h, xyzz29_g2.hip.h, jac29.hip.h), of its GLV code
 * or of the saturated formulas it falls back to (bn254_curve.hip.h) on operands the HOST chose; the raw limbs, words, flags and return values
 * of that call come back (tests/test_gpu_point_ops.py judges them with Python integers, tests/point_ref.py). The field probe hands over the
 * streams these formulas are made of, the tower probe what the pairing builds on them; this is the layer between. Record layout:
 *   operands: n records of KEAKI_POP_SLOTS slots x KEAKI_POP_SLOT_WORDS uint32_t. A lazy coordinate (nine limbs, exactly as given) fills its
 *             slot; a saturated coordinate or a scalar (eight words) uses words 0..7. Flags are the words of slot KEAKI_POP_FLAG_SLOT.
 *   out:      n records of KEAKI_POP_OUT_SLOTS slots x KEAKI_POP_SLOT_WORDS uint32_t, zero where the call wrote nothing; flags, return value
 *             and `special` are the words of slot KEAKI_POP_OUT_FLAG_SLOT.
 * The slots of every op are listed at its enumerator (in: ... -> out: ...). Point forms:
 *   X29    x, y, zz, zzz (4 lazy slots) + flag `inf`          X29G2  x.re, x.im, y.re, y.im, zz.re, zz.im, zzz.re, zzz.im (8 lazy slots) + flag `empty`
 *   J29    x, y, z (3 lazy slots)                             sat    Xyzz / Jac / Aff of Fq (one slot per coordinate) or of Fq2 (c0, c1: two slots)
 * Lazy values are residues x 2^261, saturated coordinates residues x 2^256 (canonical, < p); scalars of the ladders and of
 * KEAKI_POP_GLV_UNIFORM_DIGITS are Fr in Montgomery form, KEAKI_POP_GLV_DECOMPOSE takes k itself (canonical, < r).
 * Geometry: one record per lane, 64 lanes per workgroup, all 64 lanes run (the library pads the launch to whole waves with copies of record 0
 * and only the first n records are stored). The wave-uniform forms (KEAKI_POP_GLV_UNIFORM_DIGITS, KEAKI_POP_LADDER_UNIFORM, KEAKI_POP_LADDER_MUL2)
 * take the scalars (and negB) of the WAVE'S FIRST record for the whole wave, as the shipped kernels take one twiddle per wave, and keep their
 * digits in that wave's LDS; every lane still has its own points. KEAKI_POP_LADDER_GTAB has its 1 KB of table per lane in a workspace of the
 * context. 1 <= n <= KEAKI_POP_MAX_RECORDS; an unknown op, n out of range or a null pointer is KEAKI_ERR_BAD_ARG and launches nothing. Operand
 * bounds are the callee's own; the probe does not check them. Every op is one call with the template arguments of a shipped call site
 * (KEAKI_POP_LADDER_MUL2 builds its tables with j29_build_pair first, as its only caller does).
 * Not probed: the inline mixed addition of k_msm_accumulate_g1_u29 (not a function; making it one would change a hot kernel); fb_accumulate*
 * (tests/test_gpu_fb_digit_edges.py); the Straus kernels of fk_coset.hip and vec_update.hip (their building blocks are the ops here); the
 * branch "u29_maybe_zero fires, u29_is_zero does not" (18 in 2^29 additions; the field probe covers the two predicates themselves). */
#define KEAKI_POP_SLOTS 17
#define KEAKI_POP_SLOT_WORDS 9
#define KEAKI_POP_FLAG_SLOT 16
#define KEAKI_POP_OUT_SLOTS 50
#define KEAKI_POP_OUT_FLAG_SLOT 49
#define KEAKI_POP_MAX_RECORDS 4096
#define KEAKI_POP_FIRST_G2 KEAKI_POP_X29G2_ADD_MIXED
typedef enum {
  /* xyzz29.hip.h */
  KEAKI_POP_X29_ADD = 0,             /* in: a 0..3, b 4..7, flags a.inf, b.inf -> out: X29 0..3, flag inf */
  KEAKI_POP_X29_DBL = 1,             /* in: a 0..3, flag a.inf -> out: X29 0..3, flag inf */
  KEAKI_POP_X29_STORE = 2,           /* in: a 0..3, flag a.inf -> out: Xyzz<Fq> 0..3 */
  KEAKI_POP_X29_LOAD_STORE = 3,      /* x29_store(x29_load(.)): in: Xyzz<Fq> 0..3 -> out: Xyzz<Fq> 0..3 */
  /* jac29.hip.h, point level */
  KEAKI_POP_J29_DBL = 4,             /* in: J29 0..2 -> out: J29 0..2 */
  KEAKI_POP_J29_MADD = 5,            /* in: a 0..2, x2 3, y2 4 -> out: J29 0..2, *ratio 3 (0 when not written), flag special */
  KEAKI_POP_J29_ADDSUB = 6,          /* in: u 0..2, v 3..5 -> out: sum 0..2, diff 3..5, flag return value */
  KEAKI_POP_J29_SAT_ROUNDTRIP = 7,   /* j29_to_sat(j29_from_sat(.)): in: Jac<Fq> 0..2 -> out: Jac<Fq> 0..2 */
  KEAKI_POP_J29_BUILD_TABLE = 8,     /* j29_build_table<false> through J29ArrTable: in: Jac<Fq> 0..2 -> out: entry e (x, beta x, y) at 3e..3e+2, zfix 24 */
  KEAKI_POP_J29_BUILD_TABLE_ODD = 9, /* j29_build_table<true>, the same slots */
  KEAKI_POP_J29_BUILD_PAIR = 10,     /* in: A 0..2, B 3..5 (Jac<Fq>) -> out: TA entries 0..23, TB entries 24..47, zfix 48 */
  /* GLV */
  KEAKI_POP_GLV_DECOMPOSE = 11,      /* in: k 0 (8 words) -> out: |k1| 0 (5 words), |k2| 1 (5 words), flags neg1, neg2 */
  KEAKI_POP_GLV_FIXED_DIGITS = 12,   /* in: magnitude 0 (5 words) -> out: dig 0 (5 words), sg 1 (2 words) */
  KEAKI_POP_GLV_UNIFORM_DIGITS = 13, /* in: Fr 0 (wave's first record) -> out: the 2 x UNIFORM_DIG_STRIDE bytes as 66 words from word 0, flags neg1, neg2 */
  /* ladders: in: Jac<Fq> 0..2, Fr 3 -> out: J29 0..2, flag return value */
  KEAKI_POP_LADDER_FIXED = 14,       /* jac_scalar_mul_u29_j */
  KEAKI_POP_LADDER_GTAB = 15,        /* jac_scalar_mul_gtab_u29_j */
  KEAKI_POP_LADDER_UNIFORM = 16,     /* jac_scalar_mul_uniform_u29_j: Fr of the wave's first record */
  KEAKI_POP_LADDER_MUL2 = 17,        /* j29_build_pair, j29_mul2_uniform: in: A 0..2, B 3..5, kA 6, kB 7, flag word 2 negB (kA, kB, negB of the wave's first record) */
  /* saturated formulas of bn254_curve.hip.h over Fq: in: first point from 0, second point behind it -> out: the point from 0 */
  KEAKI_POP_XYZZ_ADD_MIXED_FQ = 18,  /* in: Xyzz 0..3, Aff 4..5 */
  KEAKI_POP_XYZZ_ADD_FQ = 19,        /* in: Xyzz 0..3, Xyzz 4..7 */
  KEAKI_POP_XYZZ_DBL_FQ = 20,
  KEAKI_POP_XYZZ_DBL_AFF_FQ = 21,    /* in: Aff 0..1 */
  KEAKI_POP_JAC_ADD_FQ = 22,         /* in: Jac 0..2, Jac 3..5 */
  KEAKI_POP_JAC_ADD_MIXED_FQ = 23,   /* in: Jac 0..2, Aff 3..4 */
  KEAKI_POP_JAC_DBL_FQ = 24,
  /* xyzz29_g2.hip.h: every op from here on lives in point_probe_g2.hip */
  KEAKI_POP_X29G2_ADD_MIXED = 25,    /* in: acc 0..7, flag acc.empty, Aff<Fq2> 8..11 -> out: X29G2 0..7, flag empty */
  KEAKI_POP_X29G2_ADD = 26,          /* in: a 0..7, b 8..15, flags a.empty, b.empty -> out: X29G2 0..7, flag empty */
  KEAKI_POP_X29G2_DBL = 27,
  KEAKI_POP_X29G2_DBL_OF_ACC = 28,
  KEAKI_POP_X29G2_STORE = 29,        /* in: a 0..7, flag a.empty -> out: Xyzz<Fq2> 0..7 */
  /* the saturated formulas over Fq2: a coordinate is two slots (c0, c1) */
  KEAKI_POP_XYZZ_ADD_MIXED_FQ2 = 30, /* in: Xyzz 0..7, Aff 8..11 */
  KEAKI_POP_XYZZ_ADD_FQ2 = 31,       /* in: Xyzz 0..7, Xyzz 8..15 */
  KEAKI_POP_XYZZ_DBL_FQ2 = 32,
  KEAKI_POP_XYZZ_DBL_AFF_FQ2 = 33,
  KEAKI_POP_JAC_ADD_FQ2 = 34,        /* in: Jac 0..5, Jac 6..11 */
  KEAKI_POP_JAC_ADD_MIXED_FQ2 = 35,  /* in: Jac 0..5, Aff 6..9 */
  KEAKI_POP_JAC_DBL_FQ2 = 36,
  KEAKI_POP_COUNT = 37
} keaki_point_op;
keaki_status keaki_hip_selftest_point_ops(keaki_hip_ctx* ctx, uint32_t op, const uint32_t* operands, size_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* KEAKI_HIP_H */
