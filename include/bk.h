/*
 * bk.h -- C ABI of the MI355X-native Multi-Krum engine (libbk.so).
 *
 * Drop-in boundary for Biscotti's verifier hot path.  The reference path is
 *
 *   Peer.VerifyUpdateKRUM          DistSys/krum.go:227-365
 *    -> KRUMValidator.computeScores  DistSys/krum.go:77-98
 *     -> KRUMValidator.getTopKRUMIndex(deltas [][]float64) []int
 *                                    DistSys/krum.go:100-166   <-- replaced
 *        (go-python: marshal n*d PyFloats, call numpy krum(deltas, clip),
 *         decode the int64 index bytes)
 *         -> krum(deltas, clip)      ML/code/logistic_validator.py:36-49
 *         -> get_krum_scores(X, g)   ML/code/logistic_validator.py:54-65
 *         (aggregate: np.mean(deltas[good_idx], 0), logistic_validator.py:51)
 *
 * A cgo shim with the same Go signature as getTopKRUMIndex calls bk_multikrum
 * (see INTEGRATION.md).  Plain pointers and sizes only; no torch, no HIP types.
 *
 * Conventions
 *   X        row-major n x d with leading dimension ld (elements), fp64 or fp32
 *            (fp32 is widened exactly; every accumulation is fp64).
 *   f        number of updates to reject ("clip"; krum.go:110 computes
 *            int(0.5*n)).  Valid iff 1 <= f < n (f = 0 makes the reference's
 *            np.argpartition raise ValueError, logistic_validator.py:45).
 *   m = n-f  number selected; k = max(0, n-f-2) neighbours summed per score.
 *   sel_idx  the m selected row indices, ASCENDING (a set: the only consumer,
 *            checkIfAccepted krum.go:47-73, tests membership).  Ties at the
 *            selection boundary resolve to the lower index; NaN scores order
 *            last (as numpy's sort/argpartition do).
 *   mean     (1/m) * sum of selected rows (fp64), the north-star aggregate.
 *
 * Errors: every entry returns 0 (BK_OK) or a negative bk_status; the message
 * is in bk_last_error() (thread-local).  Nothing aborts or throws across the
 * ABI.  Calls on one context are serialised internally; each entry selects the
 * context's device itself (goroutines migrate between OS threads).
 */
#ifndef BK_H_
#define BK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BK_ABI_VERSION 14

typedef struct bk_ctx bk_ctx;

enum bk_status {
    BK_OK = 0,
    BK_EINVAL = -1,  /* bad n, d, f, ld, dtype, pointer or mode             */
    BK_ENOMEM = -2,  /* device / pinned allocation failed                    */
    BK_EHIP = -3,    /* a HIP runtime call failed                            */
    BK_ERCCL = -4,   /* an RCCL call failed / communicator missing          */
    BK_ENOTSUP = -5  /* shape outside what this build supports (n > BK_MAX_N) */
};

enum bk_dtype { BK_F64 = 0, BK_F32 = 1 };
enum bk_where { BK_HOST = 0, BK_HOST_PINNED = 1, BK_DEVICE = 2 };

#define BK_MAX_N 16384

/* ---- library ------------------------------------------------------------ */
int bk_abi_version(void);
const char *bk_last_error(void);
/* Argument check only (no GPU needed): BK_OK or BK_EINVAL / BK_ENOTSUP. */
int bk_check_args(int64_t n, int64_t d, int64_t f);

/* ---- context: replaces KRUMValidator.initialize() (krum.go:31-44), which
 *      bound pyKRUMFunc from the module imported in pyInit (honest.go:204-258) */
int bk_create(bk_ctx **out, int device);
void bk_destroy(bk_ctx *ctx);
/* Run on a caller stream (hipStream_t passed as void*); NULL = own stream. */
int bk_set_stream(bk_ctx *ctx, void *hip_stream);
void *bk_get_stream(bk_ctx *ctx);
/* Waits for the context stream (polling it for up to BK_SPIN_US, default
 * 2000 us, then blocking), then reports whether the last Multi-Krum call
 * on it produced valid outputs: BK_EHIP when k_small's hand-off wait gave up
 * (its sel entries are then -1), BK_ERCCL when a rank of a sharded call failed
 * before the exchange (bk_multikrum_sharded_device).  The asynchronous device
 * entries report these only here and through bk_selection_margin*. */
int bk_synchronize(bk_ctx *ctx);
/* C-owned pinned staging for callers that must copy (cgo: Go pointers may not
 * be retained by C, so the shim packs [][]float64 rows here). */
int bk_stage_alloc(bk_ctx *ctx, int64_t bytes, void **pinned);
int bk_stage_free(bk_ctx *ctx, void *pinned);

/* ---- the drop-in: getTopKRUMIndex (krum.go:100-166) + numpy krum ---------
 * X on host (BK_HOST / BK_HOST_PINNED: copied H2D) or device (BK_DEVICE).
 * Biscotti's deployed shapes (n <= 128, d <= 32768: the mnist and creditcard
 * verifiers, configs A and B) cross PCIe as ONE copy and run the one-launch
 * path (k_small / k_tiny, see bk_set_small_path); a BK_HOST_PINNED batch that
 * k_tiny takes whole (n <= 16, d <= 128) is not copied at all: the kernel
 * reads it over PCIe during the (synchronous) call.  A larger host batch crosses
 * PCIe in column chunks (BK_STAGE_CHUNK_BYTES, default 256 MiB) on a copy
 * stream while the previous chunk's partial Gram runs; the chunk partials are
 * summed in chunk order, so results are deterministic.
 * Outputs are HOST pointers: sel_idx (m entries), m_out, scores (n, nullable),
 * mean_out (d, nullable).  Synchronous; an invalid call (see bk_synchronize)
 * returns its error here. */
int bk_multikrum(bk_ctx *ctx, const void *X, int where, int dtype, int64_t n, int64_t d,
                 int64_t ld, int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores,
                 double *mean_out);

/* The verifier's own input: n SEPARATE host rows (getTopKRUMIndex(deltas
 * [][]float64), krum.go:100-166 -- one slice per peer, as RPC decoded them,
 * replacing the shim's serial pack of the rows into a pinned batch,
 * krum.go:117-125's marshalling loop in the reference).  rows[i] points at
 * update i's d elements (dtype; pageable or pinned host memory, any
 * alignment); the rows are only read, during the call.  libbk packs them on
 * host threads (bk_set_host_threads) into a ring of C-owned pinned slots,
 * column chunk by column chunk, and each chunk's H2D and partial Gram start
 * as soon as it is packed.  Outputs and contract as bk_multikrum (host
 * outputs, synchronous); the selection and the mean are bitwise those of
 * bk_multikrum(BK_HOST_PINNED) on the same rows packed row-major.
 * cgo: the row pointers are Go pointers stored in C memory, which Go >= 1.21
 * allows while each row's backing array is pinned (runtime.Pinner) for the
 * call (go/bk/krum_bk.go).  A null row is BK_EINVAL. */
int bk_multikrum_rows(bk_ctx *ctx, const void *const *rows, int dtype, int64_t n, int64_t d,
                      int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores,
                      double *mean_out);
/* Host threads that pack bk_multikrum_rows' rows, the caller's included (1:
 * the caller alone; 0: the default, BK_HOST_THREADS or min(8, hardware
 * threads)).  The workers are started on the next call and sleep between
 * calls. */
int bk_set_host_threads(bk_ctx *ctx, int threads);

/* ---- incremental Multi-Krum: fold each update into the Gram as it arrives ----
 * VerifyUpdateKRUM (krum.go:227-365) appends one update per RPC and waits
 * seconds for its peers; only at the threshold or the deadline (krum.go:178-224)
 * does it sort by SourceID, optionally sample (sampleUpdates, krum.go:368-388)
 * and call Krum.  A collection takes each update when it arrives: the row is
 * uploaded into a device row store and its inner products with every row
 * already there are written into a Gram kept by arrival slot, while the
 * verifier waits for the next peer.  After the last arrival only the scores,
 * the selection and the mean remain.
 * One collection per context, serialised by the context mutex, on the context
 * stream.  It owns its buffers (row store, the fp64 Gram -- lower-triangular
 * packed, n_cap (n_cap + 1) / 2 doubles, 1 GiB at BK_MAX_N -- and a small
 * pinned ring for pageable rows): any other call on the context between two
 * adds, bk_multikrum* included, leaves it intact.
 * Arithmetic: every Gram element is an fp64 FMA sum of the products (fp32 rows
 * widened per element, so exact products, as BK_F32_EXACT) in an order that
 * depends on (d, dtype) alone -- not on how the rows were grouped into adds nor
 * on how many were resident -- without atomics: the same sequence of calls
 * gives the same bits.  bk_set_f32_mode / bk_set_f64_mode do not apply to
 * collections (no fp32-MFMA, no int8 Gram).  Against bk_multikrum on the same
 * rows in the finish's order: the selection (wherever bk_selection_margin
 * reports no near tie) and the mean are BITWISE equal; the scores agree within
 * rounding (1e-9 of the largest finite score; another summation order of the
 * Gram), with the same NaN / inf pattern.
 * Errors are BK_EINVAL (a null ctx, rows, row or required output; add or
 * finish without begin; add past n_cap; n_cap > BK_MAX_N; an out-of-range or
 * repeated slot in order; n / f outside bk_check_args) or BK_ENOMEM, and leave
 * the collection as it was before the call. */

/* Start (or restart: flushCollectedUpdates, krum.go:169-176) a collection of up to
 * n_cap rows of d elements of dtype.  Reuses the buffers of an earlier collection
 * of the same or smaller footprint. */
int bk_collect_begin(bk_ctx *ctx, int dtype, int64_t n_cap, int64_t d);
/* count >= 1 rows arrive: rows[i] points at d elements (where: BK_HOST, any
 * alignment, pageable; BK_HOST_PINNED; BK_DEVICE).  They take the next `count`
 * arrival slots; *first_slot (nullable) gets the first.  On return the rows
 * have been consumed (cgo: no pointer retained): pageable rows sit in the
 * pinned ring or on the device, pinned and device rows have been copied; the
 * upload's tail and the Gram border run asynchronously on the context stream.
 * The resident rows are read once per group of up to 8 new rows. */
int bk_collect_add(bk_ctx *ctx, const void *const *rows, int64_t count, int where,
                   int64_t *first_slot);
/* count >= 1 NOISED updates arrive: Delta and Noise separately (update.go:13-22),
 * as bk_multikrum_noised takes them, so the verifier never builds NoisedDelta on
 * the host (main.go:1524-1537, 1606-1653).  deltas[i] points at d doubles,
 * noises[i*k + j] at noise vector j of update i (d doubles; noises may be NULL
 * only when k == 0); where applies to both: BK_HOST (pageable, any alignment),
 * BK_HOST_PINNED, or BK_DEVICE (separately allocated device rows, 8-byte
 * aligned, not necessarily 16).  Update i takes arrival slot *first_slot + i and
 * the row stored there is, per element and in exactly this order (fp64, no
 * contraction),
 *     delta[c] + ((0 + v_0[c]) + v_1[c] + ... + v_{k-1}[c]) / (double)k
 * -- the bits of bk_noise_apply_device.  k == 0 means no noisers: the stored row
 * is delta bitwise (bk_multikrum_noised's rule, not the literal 0/0).
 * One k_collect_noise launch noises up to 8 arriving rows whatever k is.  Device
 * rows are read where they are, through a pointer table (no copy first).  Host
 * deltas go to their store rows as bk_collect_add uploads them, the noise
 * vectors to a device staging block owned by the collection (grown on demand,
 * released with it), and the kernel adds them in place.  One launch stages at
 * most BK_COLLECT_NOISE_STAGE_BYTES (environment, read at the call; it may lower
 * the 256 MiB default): a launch covers as many rows as fit, and a row whose k
 * vectors exceed the bound is noised in consecutive column ranges -- every
 * element is independent, so any split gives the same bits.  Then the border of
 * the new slots, as bk_collect_add's; the launches are timed under BK_K_NOISE.
 * On return every input has been consumed and no pointer is retained (the cgo
 * contract of bk_collect_add); the noise kernel and the border run on
 * asynchronously on the context stream.  Plain and noised adds may be mixed
 * freely within one collection.
 * The checks, in this order, all before any copy, launch or state change (every
 * error leaves the collection as it was): BK_EINVAL for a null ctx, null
 * deltas, count < 1, k < 0, null noises with k > 0, a bad where; BK_ENOTSUP for
 * k > BK_COLLECT_NOISE_MAX_K; then BK_EINVAL for a call without
 * bk_collect_begin, a BK_F32 collection (noise is fp64 only, as
 * bk_multikrum_noised), an add past n_cap, a null deltas[i] or noises[i*k + j]
 * (the indices named).  The checks that need no collection need no GPU.
 * Added without a change of BK_ABI_VERSION (14), as bk_set_collect_wide was. */
#define BK_COLLECT_NOISE_MAX_K 64
int bk_collect_add_noised(bk_ctx *ctx, const double *const *deltas,
                          const double *const *noises, int64_t k, int64_t count,
                          int where, int64_t *first_slot);
/* The d stored doubles of each named arrival slot, copied to the host row
 * out_rows[i] (count >= 1 of them); synchronous; fp64 collections only.  How the
 * verifier gets NoisedDelta back for the block without recomputing it.
 * BK_EINVAL: a null ctx, slots or out_rows; count < 1; a call without begin; a
 * BK_F32 collection; a slot outside 0..collected-1 (named); a null output row. */
int bk_collect_read_rows(bk_ctx *ctx, const int64_t *slots, int64_t count,
                         double *const *out_rows);
/* rows collected since the last begin (0 before any) */
int bk_collect_count(bk_ctx *ctx, int64_t *count);
/* Multi-Krum over n of the collected rows: order[i] = arrival slot of the caller's
 * row i (NULL: slots 0..count-1 in arrival order, n must equal count).  A subset
 * and any permutation are allowed: the deadline path, sampleUpdates, the sort by
 * SourceID.  Outputs and contract as bk_multikrum (host pointers, synchronous;
 * scores and mean_out nullable); indices refer to the caller's rows 0..n-1.
 * Does not consume the collection: more rows may be added and finish called
 * again.  bk_selection_margin* then reports this finish's record (d = the
 * collection's d, u_G = 2^-53).  For n <= 128 and d <= 32,768 the finish is one
 * kernel launch with no copy before or after it (bk_set_small_path(ctx, 0)
 * gives the general launch chain instead; the outputs are bitwise the same);
 * bk_set_collect_wide(ctx, 1) extends that to 32,768 < d <=
 * BK_COLLECT_WIDE_MAX_D, with the same bits. */
int bk_collect_finish(bk_ctx *ctx, const int64_t *order, int64_t n, int64_t f,
                      int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out);
/* The threshold-th update arrives and Krum runs in the same critical section
 * (krum.go:291-314): exactly bk_collect_add(ctx, &row, 1, where, first_slot)
 * followed by bk_collect_finish(ctx, order, n, f, ...), in one call.  row points
 * at d elements (where as bk_collect_add's) and takes the next arrival slot, the
 * collection's count before the call; order may name that slot, may leave it
 * out, and may be NULL (all count + 1 slots in arrival order, n = count + 1).
 * Outputs, nullable arguments and the margin record (bk_selection_margin*) are
 * the finish's; synchronous, the row consumed on return.  The collection is not
 * consumed: the row is in the store and its Gram run written, so any later add
 * or finish (batched and ragged ones included) sees the bits the two calls
 * would have left.
 * Every output -- sel, scores, mean and the margin record -- is BITWISE the
 * two-call sequence's on the same collection under the same context settings.
 * With the small path on, a finish of n <= 128, d <= 32,768 and at most 128
 * rows collected after the add, the row's copy is followed by ONE launch:
 * k_collect_arrive, the border of the new row (every Gram element the bits of
 * bk_collect_add's) in front of the one-launch finish's work items, timed under
 * BK_K_SMALL; then one wait.  Everything else (bk_set_small_path(ctx, 0), n >
 * 128, more than 128 rows collected, d > 32,768 with or without
 * bk_set_collect_wide -- but see bk_set_collect_wide_arrive -- and a BK_HOST row
 * of more than 32 KiB, where the fused call measured no faster) runs the add and
 * then the finish inside the call.
 * The checks, in this order, all before any copy, launch or state change (a
 * refused call leaves the collection as it was), with the messages of the two
 * entries: BK_EINVAL for a null ctx, a null row, a bad where, a null sel_idx;
 * a call without bk_collect_begin; an add past n_cap; then the finish's on
 * count + 1 collected rows: n outside 1..count + 1; a null order with n !=
 * count + 1; f outside bk_check_args (n = 1 included: a first-ever arrival
 * cannot finish); an out-of-range or repeated slot in order.  If the launch's
 * hand-off time-out (BK_EHIP) or a HIP error hits after the copy was queued, the
 * row does not count: the next add rewrites the slot and its Gram run.
 * Added without a change of BK_ABI_VERSION (14), as bk_collect_add_noised was. */
int bk_collect_add_finish(bk_ctx *ctx, const void *row, int where,
                          const int64_t *order, int64_t n, int64_t f,
                          int64_t *first_slot /* nullable */,
                          int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out);
/* The threshold-th update arrives as Delta and Noise: exactly
 * bk_collect_add_noised(ctx, &delta, noises, k, 1, where, first_slot) followed
 * by bk_collect_finish(ctx, order, n, f, ...), in one call.  delta points at d
 * doubles, noises[j] (j < k <= BK_COLLECT_NOISE_MAX_K) at noise vector j (d
 * doubles; noises may be NULL only when k == 0); where applies to all of them,
 * as bk_collect_add_noised's (BK_DEVICE rows 8-byte aligned, not necessarily
 * 16).  The row stored in the new slot is, per element and in this order (fp64,
 * no contraction), delta[c] + ((0 + v_0[c]) + ... + v_{k-1}[c]) / (double)k.
 * Every output -- sel, scores, mean, the margin record -- and everything a later
 * add, finish, batched or ragged finish or bk_collect_read_rows sees is BITWISE
 * the two-call sequence's on the same collection under the same settings.
 * Synchronous: every input is consumed on return, no pointer is retained, and
 * the collection is not consumed.  k == 0 is bk_collect_add_finish on delta,
 * path and bits.
 * With k >= 1, the small path on, an fp64 collection, a finish of n <= 128, d <=
 * 32,768 and at most 128 rows collected after the add, the copies (host rows:
 * the delta into its store row, the k vectors into the collection's staging
 * block; device rows: none, the kernel reads them where they are) are followed
 * by ONE launch and one wait: k_collect_arrive_noised -- the noise of the new
 * row, its border and the one-launch finish's work items -- timed under
 * BK_K_SMALL and counted in bk_collect_stats' out[3].  The k pointers travel in
 * the launch arguments (no table upload).  Everything else runs the two calls
 * inside the entry, and so do host rows of more than 32 KiB other than
 * BK_HOST_PINNED rows with k == 1: there a fused run measured no faster than
 * the sequence's fastest.
 * The checks, in this order, all before any copy, launch or state change (a
 * refused call leaves the collection as it was), with the messages of the two
 * entries: BK_EINVAL for a null ctx, a null delta, k < 0, null noises with k >
 * 0, a bad where; BK_ENOTSUP for k > BK_COLLECT_NOISE_MAX_K; BK_EINVAL for a
 * null sel_idx; then for a call without bk_collect_begin, a BK_F32 collection,
 * an add past n_cap, a null noises[j]; then the finish's on count + 1 collected
 * rows, as bk_collect_add_finish's.  If the launch's hand-off time-out (BK_EHIP)
 * or a HIP error hits after the copies were queued, the row does not count.
 * Added without a change of BK_ABI_VERSION (14), as bk_collect_add_finish was. */
int bk_collect_add_noised_finish(bk_ctx *ctx, const double *delta,
                                 const double *const *noises, int64_t k, int where,
                                 const int64_t *order, int64_t n, int64_t f,
                                 int64_t *first_slot /* nullable */,
                                 int64_t *sel_idx, int64_t *m_out,
                                 double *scores, double *mean_out);
/* The launches of this collection since the last bk_collect_begin: out[0]
 * k_border, out[1] k_border_reduce (one each per group of up to 8 added rows),
 * out[2] one-launch finishes (bk_collect_finish's k_collect_small or
 * k_collect_wide), out[3] fused arrive launches (bk_collect_add_finish's
 * k_collect_arrive, bk_collect_add_noised_finish's k_collect_arrive_noised).
 * All 0 before any begin.  No kernel id of its own: the path
 * a call took, for tests and benches.  BK_EINVAL: a null ctx or out. */
int bk_collect_stats(bk_ctx *ctx, int64_t out[4]);
/* The tiny collection (off by default): with it on, and the small path on
 * (bk_set_small_path), every call of bk_collect_add (count <= 16),
 * bk_collect_add_noised (k <= BK_COLLECT_NOISE_MAX_K), bk_collect_finish,
 * bk_collect_add_finish and bk_collect_add_noised_finish on a collection with
 * d <= 128 (either dtype; the noised forms fp64 only, as ever) that leaves at
 * most 16 rows collected is ONE launch of ONE workgroup, k_collect_tiny, with no
 * device copy call and no hand-off between workgroups: host rows (BK_HOST and
 * BK_HOST_PINNED alike, any alignment) are memcpy'd by the CPU into a mapped
 * pinned arrival block the collection owns -- 16 slots by arrival slot, each a
 * row and up to 64 noise vectors of 1 KiB -- and read from there by the kernel
 * over PCIe; BK_DEVICE rows (8-byte aligned) are read where they are through
 * pointers in the launch arguments.  A plain add is one launch for all its rows,
 * a noised add one launch per row.  n_cap may be larger than 16: what counts is
 * the rows collected after the call, so a collection begun with
 * KRUM_UPDATETHRESH and finished at the deadline qualifies.  Every other call --
 * d > 128, the 17th arrival of the same collection, a batched or ragged finish
 * -- takes the paths above, and the two mix freely: the kernel leaves the row
 * store (pad columns untouched) and the packed Gram exactly as bk_collect_add
 * leaves them.  Two fused arrivals are cut further: with rows of more than 512
 * bytes, bk_collect_add_finish (any source) and bk_collect_add_noised_finish
 * from BK_DEVICE rows take today's fused launches (k_collect_arrive,
 * k_collect_arrive_noised) -- at 16 x 128 fp64 the tiny call's runs were not
 * all below theirs, at 200-byte rows they were, nothing was measured between.
 * Every output -- sel, scores, mean, the margin record, every stored row
 * (bk_collect_read_rows) and whatever a later add, finish, batched or ragged
 * finish gives -- is BITWISE what the same calls give with the switch off, and
 * with bk_set_small_path(ctx, 0).  Checks, their order and their messages are
 * the entries' own; a refused call leaves the collection and both stats as they
 * were.  An add without a finish returns behind the launch with the rows
 * consumed (device rows: once the kernel has read them); if a launch fails
 * after a row was staged, the row does not count.  bk_collect_begin waits for
 * outstanding launches before any slot can be written again.  The launches are
 * timed under BK_K_SMALL; an add with a finish also counts in bk_collect_stats'
 * out[3] and a finish in out[2], never in out[0] or out[1].
 * bk_collect_tiny_stats: the k_collect_tiny launches since the last
 * bk_collect_begin -- out[0] adds without a finish, out[1] finishes without an
 * add, out[2] adds with a finish.  All 0 before any begin.
 * BK_EINVAL: a null ctx (either entry), a null out; neither check needs a GPU.
 * Added without a change of BK_ABI_VERSION (14), as bk_set_collect_wide was. */
int bk_set_collect_tiny(bk_ctx *ctx, int on);
int bk_collect_tiny_stats(bk_ctx *ctx, int64_t out[3]);

/* Device-resident, asynchronous on the context stream.  All pointers are
 * device pointers; d_sel_idx gets m = n-f ascending indices; d_scores (n) and
 * d_mean (d) are nullable.  A failure inside the kernels (k_small's hand-off
 * timeout) cannot be returned here: bk_synchronize and bk_selection_margin*
 * report it, and every d_sel_idx entry is -1. */
int bk_multikrum_device(bk_ctx *ctx, const void *dX, int dtype, int64_t n, int64_t d,
                        int64_t ld, int64_t f, int64_t *d_sel_idx, double *d_scores,
                        double *d_mean);
/* ---- many small problems in one call (throughput mode) ---------------------
 * `batch` independent Multi-Krum problems of one shape (n, d, f):
 * problem b is the row-major n x d matrix at X + b*stride elements (row
 * stride ld; stride >= (n-1)*ld + d).  Outputs are per problem:
 * d_sel_idx batch x (n-f), d_scores batch x n (nullable),
 * d_mean batch x d (nullable).  Device pointers, asynchronous on the
 * context stream.
 * Every output of problem b -- sel, scores, mean and its margin record -- is
 * bitwise what bk_multikrum_device gives on that problem alone under the same
 * context settings.  Within the one-launch range (n <= 128, d <= 32768, the
 * small path on) the problems share launches: k_small_batch runs k_small's
 * work items of W problems from one queue (k_tiny_batch: one workgroup per
 * problem for n <= 16, d <= 128), W bounded by the launch's partial workspace
 * (the environment variable BK_BATCH_WS_BYTES, read at the call, may lower its
 * 1 GiB default; a larger batch runs as consecutive launches).  Any other
 * shape, bk_set_small_path(ctx, 0) and batch = 1 run the single-problem device
 * path once per problem on the stream (the f32 / f64 modes and certification
 * apply per problem).  hipGraph replay does not apply.
 * A hand-off give-up in any problem of a launch invalidates the launch: every
 * d_sel_idx entry of its problems is -1 and bk_synchronize returns BK_EHIP.
 * Afterwards bk_selection_margin / _record report the record of the
 * lowest-index problem with near_tie = 1, or, if there is none, of the problem
 * with the smallest gap - err_bound; bk_selection_margin_batch gives them all.
 * BK_EINVAL: null ctx, X or d_sel_idx; batch < 1; stride too small; n, f
 * outside bk_check_args.  BK_ENOTSUP: batch > BK_MAX_BATCH.  The shape checks
 * come first and need no GPU. */
#define BK_MAX_BATCH 65536
int bk_multikrum_batch_device(bk_ctx *ctx, const void *dX, int dtype, int64_t batch, int64_t n,
                              int64_t d, int64_t ld, int64_t stride, int64_t f,
                              int64_t *d_sel_idx, double *d_scores, double *d_mean);
/* X on the host (BK_HOST / BK_HOST_PINNED), host outputs (sel_idx batch x
 * (n-f), *m_out = n-f, scores and mean_out nullable), synchronous: one H2D
 * copy of the whole batch, (batch-1)*stride + (n-1)*ld + d elements, then the
 * device entry and the copies back. */
int bk_multikrum_batch(bk_ctx *ctx, const void *X, int where, int dtype, int64_t batch, int64_t n,
                       int64_t d, int64_t ld, int64_t stride, int64_t f, int64_t *sel_idx,
                       int64_t *m_out, double *scores, double *mean_out);
/* the batch x 8 margin records of the last batched call (the layout of
 * bk_selection_margin_record, one per problem); batch must be that call's */
int bk_selection_margin_batch(bk_ctx *ctx, double *records, int64_t batch);

/* ---- many small problems, each with its own n and f, in one call -------------
 * bk_multikrum_batch with a row count n_b and an f_b PER PROBLEM: attack, f or
 * seed sweeps whose batches differ in size (the reference fixes f = int(0.5 n),
 * and n is what KRUM_UPDATETHRESH, the deadline or sampleUpdates left), the
 * verdict stages at n = 28, 42, 56 and 70 side by side, several validators in
 * one process -- one call, not one per distinct (n, f).  (Problems that share
 * rows belong to bk_collect_finish_ragged, which computes their Gram once.)
 * All problems share d, dtype and ld and lie packed in ONE row-major matrix of
 * offsets[batch] rows: problem b is rows offsets[b] .. offsets[b+1]-1 (n_b =
 * the difference, offsets[0] = 0) with f = fs[b].  The outputs are packed as
 * bk_collect_finish_ragged packs them: problem b's m_b = n_b - f_b selected
 * indices (its own rows 0..n_b-1, ascending) at d_sel_idx + sum_{c<b} m_c, its
 * n_b scores at d_scores + offsets[b] (nullable), its mean at d_mean + b*d
 * (nullable, batch x d).
 * dX and the outputs are device pointers and the call is asynchronous on the
 * context stream; offsets and fs are HOST arrays, consumed before the call
 * returns (the descriptors built from them go up through a pinned ring of the
 * context's, each slot guarded by an event, so calls queued back to back on the
 * stream never share staging).
 * Every output of problem b -- sel, scores, mean and all eight margin fields --
 * is BITWISE what bk_multikrum_device gives on that problem alone under the
 * same context settings.  Problems within the one-launch range (n_b <= 128, d
 * <= 32,768, the small path on) are grouped by ceil(n_b / 16): the single call
 * picks its kernel instantiation, its partial layout and its item counts by
 * that number and by d, so only problems that agree in it share launches.  Each
 * group of two or more runs as k_small_ragged launches of W problems -- k_small's
 * work items behind a per-problem descriptor, every output written at the
 * caller's position -- W bounded by 1,024 and by the launch's partial workspace
 * (BK_BATCH_WS_BYTES, as bk_multikrum_batch); with d <= 128 the n_b <= 16 group
 * runs as one k_tiny_ragged launch, one workgroup per problem.  A group's only
 * problem, every problem outside the range, bk_set_small_path(ctx, 0) and
 * batch = 1 run the single-problem device path in the same call (the f32 / f64
 * modes and certification apply per problem there); a call may mix all three.
 * The buffers are bk_multikrum_batch's, with their life-cycle: a single call, a
 * batched call or a collection finish between two ragged calls is unaffected
 * and affects nothing.  hipGraph replay does not apply.
 * Measured (tools/batch_ragged_bench.py): ahead of a loop of single
 * calls and of one bk_multikrum_batch_device per distinct (n, f) at every batch
 * size tried, 2 included; where all problems share one (n, f),
 * bk_multikrum_batch_device stays the faster call (the ragged one takes 1.08-
 * 1.10 x its time at 100 x 7,850 from a batch of 16, 1.27 x at a batch of 2,
 * and 1.2-2.0 x at 10 x 25: one descriptor copy per call, and a descriptor
 * read and a segment search per item).
 * A hand-off give-up in a launch invalidates the launch: every d_sel_idx entry
 * of its problems is -1, their records carry the time-out code, and
 * bk_synchronize (and the host entry) return BK_EHIP.
 * Afterwards bk_selection_margin / _record follow bk_multikrum_batch's rule,
 * and bk_selection_margin_batch(ctx, records, batch) gives the batch records in
 * the caller's problem order.  Timed under BK_K_SMALL, BK_K_H2D and BK_K_D2H.
 * The checks, in this order, all before any copy, launch or state change: a
 * bad dtype; batch < 1 (BK_EINVAL), batch > BK_MAX_BATCH (BK_ENOTSUP), d < 1,
 * ld < d (no GPU or context needed); then BK_EINVAL for a null ctx, X, offsets,
 * fs or sel (each named); offsets[0] != 0 or an n_b < 1 (the problem named);
 * then bk_check_args(n_b, d, f_b)'s status, its message behind "problem b: ";
 * then, for the host entry, a bad `where`. */
int bk_multikrum_ragged_device(bk_ctx *ctx, const void *dX, int dtype, int64_t batch,
                               const int64_t *offsets /* HOST, batch + 1 */,
                               const int64_t *fs /* HOST, batch */, int64_t d, int64_t ld,
                               int64_t *d_sel_idx, double *d_scores, double *d_mean);
/* X on the host (BK_HOST / BK_HOST_PINNED), host outputs (m_out nullable, batch
 * entries: m_out[b] = m_b; scores and mean_out nullable), synchronous: one H2D
 * copy of the (offsets[batch]-1)*ld + d elements, the device entry, the copies
 * back, then the records' error codes, as bk_multikrum_batch. */
int bk_multikrum_ragged(bk_ctx *ctx, const void *X, int where, int dtype, int64_t batch,
                        const int64_t *offsets, const int64_t *fs, int64_t d, int64_t ld,
                        int64_t *sel_idx, int64_t *m_out /* batch, nullable */, double *scores,
                        double *mean_out);
/* Host-side only; no context.  For W problems with n[] rows (1..128), NGI Gram
 * items (4 per 128 columns: 4 * ceil(d / 128)) and C mean items (ceil(d / 64);
 * 1 without a mean) each: the queue position `item` of k_small_ragged ->
 * problem *p and k_small's item number *it of that problem (it < NGI: G item;
 * it < NGI + n[p]: S item it - NGI; else M item it - NGI - n[p]).  The kernel
 * decodes with the same function.  BK_EINVAL outside the queue. */
int bk_ragged_batch_queue_item(const int32_t *n, int W, int NGI, int C, int64_t item, int *p,
                               int *it);

/* ---- many finishes over one collection in one call --------------------------
 * `batch` finishes over ONE collection in one call: problem b is Multi-Krum
 * over the n collected rows orders[b*n .. b*n+n) (arrival slots; a subset and
 * any permutation, as bk_collect_finish's order), all with the same n and f --
 * the resampled verdicts of sampleUpdates (krum.go:368-388), leave-one-out, a
 * deadline subset against the full set, a bootstrap vote per peer.  Host
 * pointers, synchronous, on the context stream under the context mutex; does
 * not consume the collection.  Outputs are per problem: sel_idx batch x (n-f)
 * (the caller's row indices 0..n-1 of that problem, ascending), *m_out = n-f,
 * scores batch x n (nullable), mean_out batch x d (nullable).
 * Every output of problem b -- sel, scores, mean and all eight margin fields --
 * is BITWISE what bk_collect_finish(ctx, orders + b*n, n, f, ...) gives on the
 * same collection under the same context settings.  Within the one-launch
 * range (n <= 128, d <= 32,768, the small path on) and for batch >= 2 the
 * problems share launches: k_collect_small_batch runs k_collect_small's work
 * items of up to 1,024 problems from one queue, reading the collection's Gram
 * and row store through each problem's order -- no Gram work, and nothing
 * uploaded but the batch x n slot numbers; a larger batch runs as consecutive
 * launches.  With bk_set_collect_wide on, 32,768 < d <= BK_COLLECT_WIDE_MAX_D
 * shares launches too (k_collect_wide_ragged on uniform descriptors), the
 * problems per launch bounded by 1,024 and by the mean bytes a launch writes,
 * batch x d doubles (the environment variable BK_COLLECT_WIDE_OUT_BYTES, read
 * at the call, may lower its 1 GiB default; a launch holds one problem at
 * least).  Any other shape, bk_set_small_path(ctx, 0) and batch = 1 run the
 * single finish once per problem.  Its buffers are its own: a bk_collect_finish,
 * bk_multikrum* or bk_multikrum_batch* between two calls is unaffected and
 * affects nothing here; a bk_collect_begin that regrows the collection and
 * bk_destroy release them.
 * A hand-off give-up in any problem of a launch invalidates the launch: every
 * sel_idx entry of its problems is -1 and the call returns BK_EHIP.
 * Afterwards bk_selection_margin / _record / _batch behave as after
 * bk_multikrum_batch: a record with an error code wins, else the lowest-index
 * problem with near_tie = 1, else the problem with the smallest gap -
 * err_bound; bk_selection_margin_batch gives them all.
 * The shape checks come first and need no GPU and no collection: batch < 1 is
 * BK_EINVAL, batch > BK_MAX_BATCH is BK_ENOTSUP.  Then, in this order,
 * BK_EINVAL for: a null ctx, orders or sel_idx; a call without
 * bk_collect_begin; n outside 1..count; f outside bk_check_args; an
 * out-of-range or repeated slot in any problem (the message names the problem
 * and the position).  Every error leaves the collection, and the last valid
 * margin state, as they were.
 * Problems that differ in n or f go to bk_collect_finish_ragged in one call. */
int bk_collect_finish_batch(bk_ctx *ctx, const int64_t *orders, int64_t batch, int64_t n,
                            int64_t f, int64_t *sel_idx /* batch x (n-f) */, int64_t *m_out,
                            double *scores /* batch x n, nullable */,
                            double *mean_out /* batch x d, nullable */);

/* ---- many finishes over one collection, each with its own n and f -----------
 * bk_collect_finish_batch with a row count n_b and an f_b PER PROBLEM: the
 * deadline subset (krum.go:178-224) next to the full set, an f sweep over the
 * same rows (krum.go:110 fixes f = 0.5 n), the deadline's verdict after each
 * arrival (the prefixes j = 2..n), leave-k-out for several k, sampleUpdates at
 * several NUM_SAMPLES -- one call, not one per distinct (n, f).
 * Problem b is Multi-Krum with f = fs[b] over the n_b = offsets[b+1] -
 * offsets[b] collected rows orders[offsets[b] .. offsets[b+1]) (arrival slots:
 * a subset and any permutation); offsets has batch + 1 entries, offsets[0] = 0.
 * Host pointers, synchronous, on the context stream under the context mutex;
 * does not consume the collection.  The outputs are packed in the caller's
 * problem order: problem b's m_b = n_b - f_b selected indices (its own row
 * indices 0..n_b-1, ascending) at sel_idx + sum_{c<b} m_c, m_out[b] = m_b
 * (nullable, batch entries), its n_b scores at scores + offsets[b] (nullable),
 * its mean at mean_out + b*d (nullable, batch x d).
 * Every output of problem b -- sel, scores, mean and all eight margin fields --
 * is BITWISE what bk_collect_finish(ctx, orders + offsets[b], n_b, fs[b], ...)
 * gives on the same collection under the same context settings.  Problems
 * within the one-launch range (n_b <= 128, d <= 32,768, the small path on) are
 * grouped by ceil(n_b / 16) -- the single finish picks its summation shapes by
 * that number, so only problems that agree in it may share a launch -- and
 * each group of two or more runs as k_collect_small_ragged launches of up to
 * 1,024 problems: k_collect_small's work items behind a per-problem descriptor,
 * every output written at the caller's position.  With bk_set_collect_wide on
 * and 32,768 < d <= BK_COLLECT_WIDE_MAX_D the grouping is the same and the
 * launches are k_collect_wide_ragged's, bounded as bk_collect_finish_batch's
 * (BK_COLLECT_WIDE_OUT_BYTES).  Every other problem, and a
 * group's only one, runs the single finish; a call may mix both.  Its buffers
 * are bk_collect_finish_batch's, with their life-cycle: nothing between two
 * calls (a single or a batched finish, bk_multikrum*, bk_collect_add) affects
 * them or is affected.
 * A hand-off give-up in a launch invalidates the launch: every sel_idx entry of
 * its problems is -1 and the call returns BK_EHIP.
 * Afterwards bk_selection_margin / _record follow bk_multikrum_batch's rule,
 * and bk_selection_margin_batch(ctx, records, batch) gives the batch records in
 * the caller's problem order.  Timed under BK_K_SMALL, BK_K_H2D and BK_K_D2H.
 * The checks, in this order, all before any launch or state change: batch < 1
 * is BK_EINVAL and batch > BK_MAX_BATCH is BK_ENOTSUP (no GPU, context or
 * collection needed); then BK_EINVAL for a null ctx, orders, offsets, fs or
 * sel_idx (named); a call without bk_collect_begin; offsets[0] != 0 or an n_b
 * outside 1..count (the problem named); then bk_check_args(n_b, d, f_b)'s
 * status, its message behind "problem b: "; then BK_EINVAL for an out-of-range
 * or repeated slot within a problem (the problem and the position named).
 * Every error leaves the collection, and the last valid margin state, as they
 * were. */
int bk_collect_finish_ragged(bk_ctx *ctx, const int64_t *orders, const int64_t *offsets,
                             const int64_t *fs, int64_t batch, int64_t *sel_idx, int64_t *m_out,
                             double *scores, double *mean_out);
/* Host-side only; no context.  For W problems with n[] rows (1..128) and C
 * mean items each (ceil(d / 64), or ceil(d / 2,048) for k_collect_wide_ragged;
 * 1 without a mean): the queue position `item` of k_collect_small_ragged ->
 * problem *p and k_collect_small's item number *it (it < n[p]: S item; else M
 * item it - n[p]).  The kernel and the host entry decode with the same
 * function.  BK_EINVAL outside the queue. */
int bk_ragged_queue_item(const int32_t *n, int W, int C, int64_t item, int *p, int *it);

/* Small batches (n <= 128, d <= 32768: Biscotti's deployed shapes, configs A
 * and B) run as ONE launch,
 * k_small: split-K Gram, reduce, scores, selection and mean pulled as work
 * items from a queue in dependency order (no co-residency assumed).  The same
 * results as the general path: selection, and the mean bitwise; scores within
 * rounding (another split of the Gram).  on = 0 forces the general path. */
int bk_set_small_path(bk_ctx *ctx, int on);
/* Opt-in (default off): the one-launch collection finishes for WIDE rows.  With
 * on != 0 (and the small path on) bk_collect_finish, bk_collect_finish_batch
 * and bk_collect_finish_ragged take one launch for n <= 128 and 32,768 < d <=
 * BK_COLLECT_WIDE_MAX_D as well: k_collect_wide keeps k_collect_small's score
 * items and queue, and its mean items stream 2,048 columns of the selected rows
 * each from the row store (k_collect_wide_ragged behind the batched and ragged
 * entries' descriptors).  Every output stays bitwise the launch chain's.
 * A call that asks for the mean takes the wide launch only up to d =
 * BK_COLLECT_WIDE_MEAN_MAX_D: the wide finish hands the mean over through
 * mapped host memory, and past that size it was measured behind the chain's
 * DMA copy (100 x 259,770 fp64: 181 us against 159; 100 x 163,850: 126 against
 * 140); a call without a mean, the verifier's own, does not depend on d (24 us
 * against 66).  bk_set_small_path(ctx, 0) still forces the chain everywhere.
 * BK_EINVAL: a null ctx.  Added without a change of BK_ABI_VERSION (14): the
 * entry is additive, and a library that lacks it fails at link or symbol
 * lookup. */
#define BK_COLLECT_WIDE_MAX_D 1048576
#define BK_COLLECT_WIDE_MEAN_MAX_D 165888 /* 81 mean items of 2,048 columns */
int bk_set_collect_wide(bk_ctx *ctx, int on);
/* Opt-in (default off), with effect only while bk_set_collect_wide is on: the
 * last arrival of a WIDE row and its finish in one launch.  With on != 0,
 * bk_collect_add_finish whose finish is in the wide one-launch range (n <= 128,
 * 32,768 < d <= BK_COLLECT_WIDE_MAX_D without a mean, <=
 * BK_COLLECT_WIDE_MEAN_MAX_D with one), with at most 128 rows collected after
 * the add and a BK_HOST_PINNED or BK_DEVICE row, is the row's copy into its
 * slot followed by ONE launch and one wait: k_collect_arrive_wide -- the
 * border of the new row spread over the grid (k_border's chunk partials into
 * the collection's partials buffer, k_border_reduce's chunk sums into the
 * Gram, every element the bits of bk_collect_add's) in front of
 * k_collect_wide's score and mean items.  Timed under BK_K_SMALL and counted
 * in bk_collect_stats' out[3], never in out[0] or out[1].  Every output --
 * sel, scores, mean, the margin record -- and everything a later add, finish,
 * batched or ragged finish or bk_collect_read_rows sees is BITWISE the
 * two-call sequence's.  Checks, their order and their messages are
 * bk_collect_add_finish's; a refused call leaves the collection and the stats
 * as they were, and a row whose launch failed does not count.  A pageable
 * (BK_HOST) row, bk_collect_add_noised_finish, bk_collect_add and the batched
 * and ragged finishes are unchanged; with the switch off every call takes
 * exactly the launches it took before.  on = 1 takes the fused launch only
 * where it was measured ahead of the sequence: a BK_HOST_PINNED row of at most
 * 320,000 bytes (40,000 fp64 columns) in a call that asks for the mean (88.0
 * against 89.8 us at 100 x 40,000; at 100 x 163,850 and beyond, from device
 * rows and without the mean it was level or behind, e.g. 58.3 against 54.3 us)
 * -- every other call of the range runs the sequence inside the entry.  on = 2
 * takes it in the whole range (for tests and measurements).  BK_EINVAL: a null
 * ctx.
 * bk_collect_wide_arrive_item: the kernel's queue, for tests -- item `item` of
 * the launch for `rows` rows collected after the add (1..128), a finish of n
 * rows with (mean != 0) or without a mean: kind 0 B (a = chunk, b = row block
 * of the border partials), 1 R (a = first Gram element of run rows - 1, b =
 * elements), 2 S (a = row), 3 M (a = mean item); counts[0..3] = the items of
 * each kind, numbered in that order.  Host-side only.  BK_EINVAL: a null
 * output, a shape outside the range, an item outside the queue.
 * Both added without a change of BK_ABI_VERSION (14), as bk_set_collect_tiny
 * was. */
int bk_set_collect_wide_arrive(bk_ctx *ctx, int on);
int bk_collect_wide_arrive_item(int64_t rows, int64_t d, int dtype, int64_t n, int mean,
                                int64_t item, int *kind, int *a, int *b, int64_t counts[4]);
/* Replay bk_multikrum_device as a hipGraph (one captured launch sequence per
 * call signature: pointers, shape, f; up to 4 cached).  The first call of a
 * signature runs eagerly, the second captures, later ones replay; graphs are
 * bypassed while per-kernel timing is on, and retired when the context's
 * workspace is reallocated.  Off by default; on = 0 frees the cached graphs. */
int bk_graph_enable(bk_ctx *ctx, int on);

/* fp32 rows (dtype BK_F32): BK_F32_EXACT (default) widens every element onto
 * the fp64 MFMA, which is exact per product and accumulates in fp64.
 * BK_F32_MFMA (BASELINE config E's "fp32 MFMA path") runs
 * v_mfma_f32_16x16x4_f32 at twice the fp64 rate: products are rounded to fp32
 * and summed in fp32 within one K1 workgroup segment, and the segments'
 * partials are summed in fp64.  Tolerance, as SURVEY.md §8(d) restates it for
 * config E: the selection matches wherever the score gap at the boundary
 * exceeds the fp32 Gram error bound (~2 k gamma_d max|x_i|^2).  The mean is
 * unchanged (fp64 accumulation of the fp32 rows).  No effect on fp64 rows. */
enum bk_f32_mode {
    BK_F32_EXACT = 0,
    BK_F32_MFMA = 1,
    BK_F32_CERTIFIED = 2,
    BK_F32_I8 = 3,
    BK_F32_I8_CERTIFIED = 4,
    BK_F32_I8X2 = 5,
    BK_F32_I8X2_CERTIFIED = 6
};
/* BK_F32_I8: the Gram from exact int8 digit slices on v_mfma_i32_32x32x32_i8
 * (bk_i8.hip, K1i8; the Ozaki scheme).  Per range of columns (at least 8,
 * each row's slice <= 128 KiB) every row is scaled by a power of two >= its max |x| and cut into three
 * signed 7-bit digits; the six digit products of weight >= 2^-26 accumulate
 * exactly in int32 and combine exactly in fp64, so each range's partial is
 * exact for the truncated digits and the result deterministic.  The dropped
 * digits bound every Gram element's error ABSOLUTELY by
 *     sum_r 2^-21 (2 S_r L1_r + 2.03 d_r S_r^2)
 * (S_r the largest row scale, L1_r the largest ||x_i||_1 of range r, d_r its
 * columns), carried in the packed record and added to the selection margin's
 * bound: a selection that differs from the reference's comes with near_tie = 1.
 * Far tighter than the fp32 MFMA's gamma_d (config E: ~1e-4 against ~1.6e-2 of
 * max |x_i|^2) and several times faster.  Rows must be 16-B aligned (ld % 4 ==
 * 0, aligned base) and d >= 64; other batches take the exact path.  A
 * non-finite input makes the bound +inf (a near tie). */
/* BK_F32_I8X2: the same slicing with TWO digits (x / s = a0/64 + a1/2^13 +
 * rho, |rho| <= 2^-14) and the three digit products of weight >= 2^-19 (A0
 * A0^T, A0 A1^T, A1 A0^T) on 128 x 256 output tiles: half the products and
 * two thirds of the digit bytes of BK_F32_I8, under the absolute bound
 *     sum_r 2^-14 (2 S_r L1_r + 1.0001 d_r S_r^2)
 * (~2^7 looser than BK_F32_I8's; config E: still ~20x below its boundary
 * gap).  BK_F32_I8X2_CERTIFIED re-runs a near tie exact. */
/* BK_F32_CERTIFIED: the fp32 MFMA, then -- only when the selection margin
 * (bk_selection_margin) does not clear the fp32 bound -- the exact path on the
 * same device-resident batch, whose outputs replace the first run's.  Never
 * silently different from the reference where the exact path is not; the
 * entries become synchronous (the decision reads the margin on the host).
 * Only a Gram taken on the fp32 MFMA is re-run (the n <= 128 one-launch path
 * is always exact).  bk_group_multikrum honours it when it is set on the
 * group's contexts (bk_group_ctx): a near tie re-runs every device's shard
 * exact from device memory, then exchanges and finishes again. */
int bk_set_f32_mode(bk_ctx *ctx, int mode);
/* fp64 rows (dtype BK_F64): BK_F64_EXACT (default) runs the fp64 MFMA;
 * BK_F64_I8 takes the Gram from the same exact int8 digit slices as BK_F32_I8
 * (the digits of an fp64 row: every slicing step exact, only the remainder
 * past the third digit dropped) under the same absolute error bound;
 * BK_F64_I8_CERTIFIED re-runs the fp64 MFMA on a near tie, so its selected
 * set is always the reference's.  The mean is unchanged (K4 reads the fp64
 * rows).  Rows must be 16-B aligned (even ld) and d >= 64. */
enum bk_f64_mode {
    BK_F64_EXACT = 0,
    BK_F64_I8 = 3,
    BK_F64_I8_CERTIFIED = 4,
    BK_F64_I8X2 = 5,          /* the two-digit slicing of BK_F32_I8X2 on fp64 rows */
    BK_F64_I8X2_CERTIFIED = 6
};
int bk_set_f64_mode(bk_ctx *ctx, int mode);
/* BK_F32_I8_CERTIFIED: the same contract on the int8-sliced Gram.
 * exact re-runs BK_F32_CERTIFIED / BK_F32_I8_CERTIFIED have made on this context */
int64_t bk_certified_reruns(bk_ctx *ctx);

/* ---- selection margin: where the selection may legitimately differ from the
 * reference's (SURVEY.md §7 "Hard parts", §8(d); logistic_validator.py:45,
 * 59-63: argpartition over BLAS-rounded scores).  Every Multi-Krum call
 * (any entry) leaves on its context, computed on the device by the finish:
 *   gap       = s[rank m] - s[rank m-1], the lowest rejected score minus the
 *               highest selected one (+inf across a finite -> NaN boundary)
 *   err_bound = 2 (e_here + e_ref),  e = 4 k M' (gamma_{d+2}(u_G) + 2u + gamma_k(u))
 *               with M' >= max_i ||x_i||^2 (finite rows), u = 2^-53, u_G the
 *               Gram's unit roundoff here (2^-53, or 2^-24 once any of its
 *               columns ran on the fp32 MFMA), gamma_j(u) = j u / (1 - j u),
 *               d the Gram's total column count (after a multi-GPU exchange
 *               too; both come from the packed record's trailing pair), k =
 *               n - f - 2
 *   near_tie  = !(gap > err_bound); a record without a column count (d < 1,
 *               e.g. a caller's own packed Gram) has err_bound = +inf and
 *               near_tie = 1
 * Any fp64 computation of the reference formula in any summation order --
 * numpy's BLAS included -- gives scores within e of the exact ones, so when
 * near_tie = 0 the reference provably selects exactly sel_idx.  near_tie = 1
 * means the boundary is within rounding (or an exact tie, e.g. k = 0 where every
 * score is 0): the lower-index tie rule decided, and numpy's choice may differ.
 * Reads the record of the last call (synchronizes the context stream); returns
 * the errors bk_synchronize does when that call's outputs are invalid. */
int bk_selection_margin(bk_ctx *ctx, double *gap, double *err_bound, int *near_tie);
/* the whole record: {gap, err_bound, near_tie, M, s_lo, s_hi, d, k} (8 doubles) */
int bk_selection_margin_record(bk_ctx *ctx, double *record);

/* ---- dimension-sharded stages (one process / device per column shard) ----
 * Packed upper-triangle Gram: bk_upper_elems(n) doubles = the 64x64 upper
 * sub-tiles, then a trailing pair: the column count, and how many of those
 * columns were accumulated on the fp32 MFMA.  Summing the packed partials of
 * all shards (trailing pairs included) gives the Gram of the full batch, its
 * total d and its unit roundoff, which the selection margin uses. */
int64_t bk_upper_elems(int64_t n);
/* On failure d_upper's trailing pair is set to NaN (best effort): a caller
 * that still joins its exchange, so its peers are not left waiting, hands
 * every rank a record that bk_finish_device marks invalid (BK_ERCCL from
 * bk_synchronize / bk_selection_margin*). */
int bk_gram_upper_device(bk_ctx *ctx, const void *dX, int dtype, int64_t n, int64_t d,
                         int64_t ld, double *d_upper);
/* Scores + selection from a (summed) packed Gram, then the mean of this
 * shard's d columns of dX (d_mean nullable). */
int bk_finish_device(bk_ctx *ctx, const double *d_upper, const void *dX, int dtype, int64_t n,
                     int64_t d, int64_t ld, int64_t f, int64_t *d_sel_idx, double *d_scores,
                     double *d_mean);

/* ---- RCCL (one rank per process, xGMI) ------------------------------------ */
#define BK_UNIQUE_ID_BYTES 128
int bk_comm_unique_id(void *id_out /* BK_UNIQUE_ID_BYTES */);
int bk_comm_init(bk_ctx *ctx, int nranks, int rank, const void *id /* BK_UNIQUE_ID_BYTES */);
/* 0: ncclAllReduce(sum) of the packed Gram (default);
 * 1: deterministic -- ncclAllGather of the partials + fixed rank-order sum;
 * 2: the all-reduce overlapped with the Gram -- the packed upper cut into
 *    pieces by rows (BK_OVERLAP_PIECES, 2..8, default 2, each ~0.6 of the one
 *    before), each piece computed by its own launches and all-reduced on a
 *    communication stream while the next computes.  Every output is bitwise
 *    mode 0's (the pieces run the same segments / (tile, range) items; the
 *    sum is element-wise).  Applies where the Gram splits into such pieces
 *    (K1i8, and the K1 plans whose workgroups each stay in one piece: n >=
 *    ~2048, config E); elsewhere (config D's n = 512 plan) mode 0 runs.
 * Set on every rank alike. */
int bk_comm_set_mode(bk_ctx *ctx, int mode);
/* Partial Gram of the local column shard -> all-reduce -> scores/selection
 * (redundant on every rank) -> mean of the local columns.  Async on stream. */
/* d_local = 0 is allowed (an empty trailing shard: dX_local, ld and
 * d_mean_local unused); the rank still joins the exchange.
 * No rank strands its peers in the collective: the first call of a signature
 * (n, f, dtype, exchange mode) allocates the workspace and agrees on a status
 * word (one extra 8-B all-reduce and a host wait), so an allocation failure
 * is an error on every rank (BK_ERCCL on the peers); a later failure before
 * the exchange poisons the rank's partial and the rank still joins, so every
 * rank's bk_synchronize reports BK_ERCCL and the failing rank returns its own
 * error. */
int bk_multikrum_sharded_device(bk_ctx *ctx, const void *dX_local, int dtype, int64_t n,
                                int64_t d_local, int64_t ld, int64_t f, int64_t *d_sel_idx,
                                double *d_scores, double *d_mean_local);
/* the communicator's size and this rank (ncclCommCount / ncclCommUserRank);
 * nranks = 0 when bk_comm_init was not called */
int bk_comm_size(bk_ctx *ctx, int *nranks, int *rank);
/* exchanges of the packed Gram made on this context, and the bytes this rank
 * put into them (all-reduce: bk_upper_elems(n) * 8 each; all-gather: x nranks) */
int bk_comm_stats(bk_ctx *ctx, int64_t *exchanges, double *bytes);

/* ---- one process, G GPUs: the Go verifier's form ------
 * A verifier is ONE process holding [][]float64 in host memory
 * (VerifyUpdateKRUM, krum.go:227-365).  A group owns one context per device
 * and splits the columns like bk_multikrum_sharded_device: each device copies
 * its column shard over its own PCIe link, computes its partial Gram, the
 * partials are summed, every device scores and selects (identically) and
 * writes the mean of its columns into mean_out.
 *   mode BK_GROUP_ALLREDUCE:  ncclAllReduce over one communicator
 *                             (ncclCommInitAll), devices must be distinct;
 *   BK_GROUP_DETERMINISTIC:   ncclAllGather + fixed rank-order sum;
 *   BK_GROUP_HOST_EXCHANGE:   partials through pinned host memory, summed in
 *                             fixed rank order -- no RCCL; any device list,
 *                             repeats allowed (bitwise equal to DETERMINISTIC).
 * devices may be NULL (0..ngpus-1). */
typedef struct bk_group bk_group;
enum bk_group_mode { BK_GROUP_ALLREDUCE = 0, BK_GROUP_DETERMINISTIC = 1, BK_GROUP_HOST_EXCHANGE = 2 };
int bk_group_create(bk_group **out, int ngpus, const int *devices, int mode);
void bk_group_destroy(bk_group *g);
int bk_group_size(const bk_group *g);
/* bk_multikrum's contract (host X: BK_HOST or BK_HOST_PINNED; host outputs;
 * synchronous) over the group's devices.  shard_bounds: GPU r owns columns
 * [r*per, min(d, (r+1)*per)), per = ceil(d/G) rounded up to 8. */
int bk_group_multikrum(bk_group *g, const void *X, int where, int dtype, int64_t n, int64_t d,
                       int64_t ld, int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores,
                       double *mean_out);
/* per-device context (timing, streams); r in [0, G) */
bk_ctx *bk_group_ctx(bk_group *g, int r);

/* ---- synthetic batches (spec: DESIGN.md "Synthetic inputs") --------------
 * Rows [0,n) x columns [c0, c0+d_local) of the n x d_total batch, generated on
 * the device bit-identically to oracle/krum_oracle.c and the numpy spec. */
#define BK_SYNTH_FP32ROUND 1
int bk_synth_fill_device(bk_ctx *ctx, void *dX, int dtype, int64_t n, int64_t d_local,
                         int64_t ld, int64_t c0, int64_t d_total, uint64_t seed, int64_t nbyz,
                         double mu_scale, double byz_scale, double sigma, int flags);

/* ---- the steps either side of Multi-Krum --- */

/* Block aggregation of the accepted updates -- replaces the update loop of
 * Honest.createBlock, DistSys/honest.go:360-375 (pulledGradientM.Add per
 * accepted update, in blockUpdates order):
 *     for r = 0 .. m-1:  global[c] = global[c] + X[idx[r]][c]
 * sequential fp64 adds in idx order, bit-identical to the Go loop.  idx lists
 * the accepted rows in the caller's update order (duplicates allowed); m = 0
 * leaves global unchanged.  The stake bookkeeping (+-STAKE_UNIT) stays above
 * the boundary.  Device variant: d_idx entries must lie in [0, n) (not checked
 * on the device); m <= BK_MAX_N. */
int bk_aggregate_device(bk_ctx *ctx, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                        const int64_t *d_idx, int64_t m, double *d_global);
/* Host-buffer variant for the Go miner: X as in bk_multikrum (where), idx and
 * global (in/out, d entries) in host memory; idx is range-checked (BK_EINVAL). */
int bk_aggregate(bk_ctx *ctx, const void *X, int where, int dtype, int64_t n, int64_t d,
                 int64_t ld, const int64_t *idx, int64_t m, double *global);

/* Secure-aggregation quantised sum -- updateFloatToInt (DistSys/kyber.go:698-710)
 * of each accepted update, summed as the miners' share aggregation does before
 * recovery (honest.go:401-409, 442-502), and updateIntToFloat (kyber.go:745-757):
 *     d_sum[c]       = sum_r int64(X[idx[r]][c] * 10^precision)   (int64, wrapping)
 *     d_sum_float[c] = float64(d_sum[c]) / 10^precision           (nullable)
 * int64(float64) follows Go on amd64: truncation toward zero, NaN and
 * out-of-range values give INT64_MIN.  0 <= precision <= 18 (Biscotti uses
 * PRECISION = 4, main.go:45). */
int bk_quantized_sum_device(bk_ctx *ctx, const void *dX, int dtype, int64_t n, int64_t d,
                            int64_t ld, const int64_t *d_idx, int64_t m, int precision,
                            int64_t *d_sum, double *d_sum_float);

/* ---- the miner's block, added to as the updates arrive -------------------- */

/* A miner receives its updates one RPC at a time (Peer.RegisterUpdate ->
 * processUpdate -> addBlockUpdate, DistSys/main.go:375, :1206-1235,
 * honest.go:330-334) and createBlock adds the accepted ones in arrival order
 * (honest.go:346-388).  The block family does each add when its update
 * arrives, so the last arrival waits for its own row only.  One block per
 * context, serialised by the context mutex on the context stream; it owns its
 * buffers, is independent of a collection on the same context, and any other
 * call between two adds leaves it intact (and it them).
 *
 * bk_block_begin: start (or restart, reusing the buffers) a block of rows of
 * `dtype` with d elements from the gradient global_w (d doubles at `where`:
 * BK_HOST, BK_HOST_PINNED or BK_DEVICE; consumed on return).  precision -1: no
 * quantised sum; 0..18: a running int64 sum of int64(row * 10^precision) is
 * kept next to the fp64 one, cleared here. */
int bk_block_begin(bk_ctx *ctx, int dtype, int64_t d, const double *global_w, int where,
                   int precision);
/* count >= 1 rows arrive (rows[i]: d elements at `where`, as bk_collect_add's:
 * pageable with any alignment, pinned, or device rows aligned to their element
 * size) and take the next `count` arrival slots (*first_slot, nullable: the
 * first of them).  For each row with accepted[i] != 0 (accepted NULL: all), in
 * the order given,
 *     global[c] = global[c] + (double)rows[i][c]        (fp64, no contraction)
 * and, with precision >= 0,
 *     q[c] += int64((double)rows[i][c] * 10^precision)  (wrapping; Go's int64())
 * Rejected rows are counted and never read (honest.go:367-370).  Every input is
 * consumed on return. */
int bk_block_add(bk_ctx *ctx, const void *const *rows, const uint8_t *accepted, int64_t count,
                 int where, int64_t *first_slot);
/* The rows added since the begin, and how many of them were accepted. */
int bk_block_count(bk_ctx *ctx, int64_t *added, int64_t *accepted);
/* The block so far, synchronously; it is not consumed (the deadline path
 * finishes, more rows may arrive, and it finishes again).  global_out (d
 * doubles, host) is bitwise bk_aggregate of the stacked rows with idx the
 * accepted slots in arrival order and the begin's global_w; qsum_out and
 * qsum_float_out (nullable, d entries each, host) are bitwise
 * bk_quantized_sum_device on the same rows and idx -- asking for either on a
 * block begun with precision -1 is BK_EINVAL. */
int bk_block_finish(bk_ctx *ctx, double *global_out, int64_t *qsum_out, double *qsum_float_out);
/* The last arrival (the NUM_SAMPLES / 2-th of main.go:1226-1231): exactly
 * bk_block_add(ctx, &row, &accepted, 1, where, first_slot) followed by
 * bk_block_finish, bitwise, in one call -- and in one launch where the
 * gradient is small enough for the kernel's own stores into mapped host memory
 * to beat the copy back (bk_block_stats). */
int bk_block_add_finish(bk_ctx *ctx, const void *row, int accepted, int where, int64_t *first_slot,
                        double *global_out, int64_t *qsum_out, double *qsum_float_out);
/* Launches since the begin: out[0] add launches (one per group of up to 8
 * arrivals with an accepted row), out[1] fused add-finish launches, out[2]
 * launches that read their rows from mapped host memory (no copy call), out[3]
 * finishes served without a D2H copy call.
 *
 * Errors of the family: BK_EINVAL for a null ctx or required pointer, count <
 * 1, a bad where or dtype, d < 1, precision outside -1..18 (none of these needs
 * a block or a GPU); then for add, count, finish or stats without begin, a null
 * rows[i] (named) and more than BK_MAX_N rows in total; BK_ENOMEM for an
 * allocation failure.  All checks precede any copy, launch or state change: a
 * refused call leaves the block as it was.  A launch group reads the running
 * sums and writes a second copy of them, which becomes current once the launch
 * is queued: after a HIP error the group's rows do not count and the sums are
 * unchanged.  The launches are timed under BK_K_AGGREGATE.  Added without a
 * change of BK_ABI_VERSION (14), as bk_set_collect_wide was. */
int bk_block_stats(bk_ctx *ctx, int64_t out[4]);

/* ---- secure aggregation: miner shares, their sum and recovery -------------- */

/* With SECURE_AGG (DistSys/main.go:151, the reference's default) a miner never
 * holds a Delta: a client cuts its quantised Delta into polynomials of
 * poly_size coefficients (makePolynomialMap, kyber.go:712-743; the last may be
 * shorter) and sends each miner the polynomials' values at that miner's share
 * points; the miner sums the parts of the agreed node list and the leader
 * recovers the summed polynomials.  Share s sits at x = s - 10
 * (pointToHashVal, kyber.go:677-695).  The bn256 commitments and witnesses are
 * not part of this family.
 *
 * Layout: y_out and every part are int64 [chunk][share]; chunks =
 * bk_shares_chunks(d, poly_size) = ceil(d / poly_size) (-1 for a bad d or
 * poly_size); a miner's part holds `held` consecutive shares per chunk (shares
 * [held m, held (m + 1)) of miner m, extractMinerSecret, kyber.go:205-242).
 *
 * bk_shares_generate: y_out[chunk][s], s < total_shares, is
 * createShareAndWitness's evaluatedValue (kyber.go:579-646) bit for bit:
 *     c_j = int64(delta[chunk poly_size + j] * 10^precision)     (Go's int64())
 *     y   = sum_j int64(pow(x, j) * float64(c_j))                (wrapping)
 *     y  += int64(r), r what dividePolynomial (kyber.go:768-793) leaves in
 *           place 0 of the float coefficients, c_0 replaced by
 *           float64(int64(float64(c_0)) - y), divided by (X - x)
 * delta (d doubles) and y_out are both at `where`.  pow(x, j) is taken as the
 * exact integer power (exact in fp64 for these x and j).
 *
 * bk_shares_begin: the miner's store of up to n_cap parts of chunks x held
 * int64 (emptied; the own aggregate forgotten).  bk_shares_add: one part (at
 * `where`) takes the next slot (*slot, nullable).  bk_shares_sum: the
 * element-wise wrapping int64 sum of the listed slots (each at most once, host
 * array) stays on the device as the context's own aggregate and is copied to
 * sum_out (host, nullable): the reply to GetMinerPart (main.go:459-485).
 *
 * bk_shares_recover: parts[i] (at `where`; NULL, at most one: the own
 * aggregate, whose d, poly_size and held must be the call's) holds held[i]
 * shares per chunk, and xs (host) the sum(held) = S nodes in part order:
 * distinct, each in [-10, 53], poly_size <= S <= 64.  Per chunk the integer
 * polynomial through the first poly_size points is recovered exactly (Newton
 * divided differences in 128-bit integers, every division exact) and checked
 * modulo 2^64 against all S points.  A chunk is bad if a division leaves a
 * remainder, a coefficient does not fit int64 or a point is not reproduced: its
 * outputs are 0 and it is counted in *bad_chunks (host), the call still
 * BK_OK.  coef_out (nullable, d int64), delta_out (nullable, d doubles:
 * float64(coef) / 10^precision, updateIntToFloat kyber.go:745-757) and
 * global_out (d doubles: global_w + that, honest.go:408-409) are at `where`,
 * as global_w is; the short last chunk's surplus coefficients are dropped
 * (honest.go:486-490).
 *
 * bk_shares_stats: since the context was made, out[0] kernel launches (one per
 * generate, sum and recover), out[1] copy calls, out[2] calls that reached the
 * device, out[3] bad chunks.
 *
 * Every entry is synchronous.  Device pointers are 8-byte aligned.  Errors:
 * BK_EINVAL for a null ctx first, then (no state or GPU needed) a null required
 * pointer, a bad where, d outside [1, 2^30], poly_size outside [1, 10],
 * total_shares outside [poly_size, 64], precision outside [0, 18], held
 * outside [1, 64], n_cap outside [1, BK_MAX_N], count < 1, nparts outside
 * [1, 64], a bad held[i], S or xs[i] (named), two null parts; then add, count
 * or sum without begin, a full store, a slot out of range or listed twice, a
 * null part without a matching own aggregate.  A refused call changes nothing.
 * The launches carry no timing id.  Added without a change of BK_ABI_VERSION
 * (14), as bk_block_* was. */
#define BK_SHARES_MAX_POLY   10
#define BK_SHARES_MAX_POINTS 64
int64_t bk_shares_chunks(int64_t d, int poly_size);
int bk_shares_generate(bk_ctx *ctx, const double *delta, int where, int64_t d, int precision,
                       int poly_size, int total_shares, int64_t *y_out);
int bk_shares_begin(bk_ctx *ctx, int64_t d, int poly_size, int held, int64_t n_cap);
int bk_shares_add(bk_ctx *ctx, const int64_t *part, int where, int64_t *slot);
int bk_shares_count(bk_ctx *ctx, int64_t *count);
int bk_shares_sum(bk_ctx *ctx, const int64_t *slots, int64_t count, int64_t *sum_out);
int bk_shares_recover(bk_ctx *ctx, const int64_t *const *parts, const int *held, const int64_t *xs,
                      int nparts, int where, int64_t d, int poly_size, int precision,
                      const double *global_w, int64_t *coef_out, double *delta_out,
                      double *global_out, int64_t *bad_chunks);
int bk_shares_stats(bk_ctx *ctx, int64_t out[4]);   /* launches, copies, calls, bad chunks so far */

/* ---- polynomial commitments in bn256 G1 ----------------------------------- */

/* The commitments a peer computes in an iteration (DistSys/kyber.go): the
 * curve is y^2 = x^3 + 3 over GF(p), p =
 * 65000549695646603732796438742359905742825358107623003571877145026864184071783,
 * of prime order n =
 * 65000549695646603732796438742359905742570406053903786389881062969044166799969.
 * A point is the 64 bytes of pointG1.MarshalBinary: affine x, then y, 32 bytes
 * each, big-endian; infinity is 64 zero bytes.  The arithmetic is in integers,
 * so every output is the reference's bit for bit whatever the order of the
 * additions.
 *
 * bk_commit_set_key: the context's resident key PKG1 (pk: count x 64 bytes,
 * host).  Every point is unmarshalled and validated on the device -- a
 * coordinate >= p or a point off the curve refuses the key (BK_EINVAL,
 * bk_last_error names the smallest such index) and leaves the resident key as
 * it was -- and kept with its multiples 1 .. 8 (512 bytes per point).
 * bk_commit_key_count: the resident key's points (0: none).
 *
 * bk_commit_msm: createCommitment(scalars, PKG1[key_first : key_first + n])
 * (kyber.go:533-562) = sum_i SetInt64(scalars[i]) PK[key_first + i], where
 * SetInt64(v) = v mod n.  scalars (n int64) and out64 are at `where`.
 * bk_commit_verify: verifyCommitment (kyber.go:564-577): *ok (host) = 1 if that
 * sum's 64 bytes equal committed64 (at `where`), else 0.
 *
 * bk_commit_generate: the commitments of generateMinerSecretShares
 * (kyber.go:456-482) for an update of d entries given as delta (d doubles,
 * quantised as bk_shares_generate quantises: int64(delta * 10^precision) by
 * Go's conversion) or as q (d int64 taken as they are, e.g. q_out of
 * bk_grad_*); exactly one of the two is non-NULL.  With chunks =
 * bk_shares_chunks(d, poly_size):
 *   commit_out   64 bytes: createCommitment(update, PKG1)
 *   chunk_out    chunks x 64: fillPolynomialMap's commitment (kyber.go:172-202)
 *                of chunk c, its coefficient j on PK[c poly_size + j]
 *   witness_out  chunks x total_shares x 64: createShareAndWitness's witness
 *                (kyber.go:579-646) of chunk c at share s (x = s - 10): the
 *                commitment, on the chunk's key points, of the int64 quotient
 *                of the chunk's float polynomial by (X - x) as
 *                dividePolynomial leaves it
 * Each output may be NULL, not all three; inputs and outputs are at `where`.
 *
 * bk_commit_stats: since the context was made, out[0] kernel launches, out[1]
 * copy calls, out[2] calls that reached the device; out[3] the resident key's
 * points.
 *
 * Every entry is synchronous.  Device pointers are 8-byte aligned (points: any
 * alignment).  Errors, checked in this order: BK_EINVAL for a null ctx, a null
 * required pointer (both or neither of delta and q), a bad where, count, n or d
 * outside [1, 2^22], key_first outside [0, 2^22]; BK_ENOTSUP for precision
 * outside [0, 18], poly_size outside [1, BK_SHARES_MAX_POLY], total_shares
 * outside [poly_size, 64]; BK_EINVAL for no output requested; then BK_EINVAL
 * for no resident key, key_first + n or d past the key, an invalid key point.
 * A refused call changes nothing.  The launches carry no timing id.  Added
 * without a change of BK_ABI_VERSION (14), as bk_shares_* was. */
int bk_commit_set_key(bk_ctx *ctx, const uint8_t *pk, int64_t count);
int bk_commit_key_count(bk_ctx *ctx, int64_t *count);
int bk_commit_msm(bk_ctx *ctx, const int64_t *scalars, int where, int64_t n, int64_t key_first,
                  uint8_t *out64);
int bk_commit_verify(bk_ctx *ctx, const int64_t *scalars, int where, int64_t n, int64_t key_first,
                     const uint8_t *committed64, int *ok);
int bk_commit_generate(bk_ctx *ctx, const double *delta, const int64_t *q, int where, int64_t d,
                       int precision, int poly_size, int total_shares, uint8_t *commit_out,
                       uint8_t *chunk_out, uint8_t *witness_out);
int bk_commit_stats(bk_ctx *ctx, int64_t out[4]);   /* launches, copies, calls, key points */

/* The gradient step -- computeUpdate -> oneGradientStep (DistSys/
 * honest.go:165-200, 284-324): privateFun of ML/code/logistic_model.py:92-140
 * (creditcard) or ML/Pytorch/client_obj.py:73-77 -> client.py:38-65 (the torch
 * softmax model), followed by updateFloatToInt (honest.go:183).  A context
 * holds ONE resident training set, the peer's shard, in buffers of its own: no
 * bk_grad* call touches an evaluation set, a validation set or a live round.
 *   bk_grad_set_logistic  X nn x d fp64 (row stride ldx), y the nn labels.
 *   bk_grad_set_softmax   X nn x d_in fp32 (row stride ldx), y int32 labels in
 *                         [0, n_classes), 2 <= n_classes <= 16; the model has
 *                         d = n_classes (d_in + 1) entries (W row-major, then b).
 *   bk_grad_clear         empties the set.
 * The two gradient calls are synchronous.  `where` (BK_HOST, BK_HOST_PINNED or
 * BK_DEVICE) holds for ww, noise, delta_out and q_out together, d entries
 * each.  idx is a HOST array of count row numbers of the set, taken in the
 * order given, repeats allowed (the caller draws them, as np.random.choice and
 * the shuffled loader do); NULL: rows 0 .. nn-1 (count is ignored).  noise
 * (nullable) is getNoise(iteration) as the caller computed it.  precision < 0:
 * no quantisation (q_out must be NULL); else q_out[j] (nullable) =
 * int64(delta_out[j] * 10^precision) by bk_quantized_sum_device's rule.
 * loss_out / norm_out are host scalars, nullable.
 *   bk_grad_logistic  z_i = the fp64 FMA chain over k ascending from +0.0 of
 *     X[r_i][k] ww[k] (bk_eval's dot), t_i = y_i z_i, res_i = -y_i / (1 +
 *     e^{t_i}); S_j = the sum over tiles of 256 batch positions, ascending, of
 *     each tile's FMA chain over its positions ascending from +0.0 of
 *     X[r_i][j] res_i; delta_j = -alpha (S_j / batch_size + lammy ww_j)
 *     [+ noise_j], every operation rounded on its own.  batch_size is the
 *     reference's divisor, independent of count.  loss = sum logaddexp(0,
 *     -t_i) + 0.5 lammy ww.ww.
 *   bk_grad_softmax   ww rounded to fp32 as bk_eval stages it; logits in fp64
 *     (k ascending, plus the bias), p = softmax over c ascending, r_ic = p_ic -
 *     [y_i = c]; G_ck = (sum over tiles of the chains of r_ic x_ik) / count,
 *     gb_c likewise with x = 1; norm = sqrt of the sum of all squares (entry e
 *     in lane e mod 256's sum, then a fixed tree); every entry times
 *     max_norm / (norm + 1e-6) where that is below 1; delta = -g [+ noise].
 *     loss = the mean cross-entropy; norm_out: the norm before clipping.
 * A NaN in ww gives an all-NaN delta_out and BK_OK.  The results never depend
 * on the grid or on timing.
 *   bk_grad_stats  out[0]: kernel launches (one per logistic call, two per
 *                  softmax call), out[1]: gradient calls, since the context
 *                  was made.
 * Checked in this order, before any copy or launch: BK_EINVAL for a null ctx,
 * ww or delta_out or a bad where; for precision > 18 or q_out with precision <
 * 0; for batch_size < 1 / a max_norm that is not finite and positive; for no
 * resident set or one of the other kind; for count < 1 with idx; for an idx
 * entry outside [0, nn) (its position named); BK_ENOTSUP for a batch of more
 * than 65,536 rows.  bk_grad_set_*: BK_EINVAL for nn < 1, d < 1, ldx < d,
 * n_classes < 2, a null X or y, a label outside [0, n_classes) (the sample
 * named); then BK_ENOTSUP for nn > 2^31, n_classes > 16, d (d_in) > 32,768.
 * Added without a change of BK_ABI_VERSION (14). */
int bk_grad_set_logistic(bk_ctx *ctx, const double *X, int64_t nn, int64_t d, int64_t ldx,
                         const double *y);
int bk_grad_set_softmax(bk_ctx *ctx, const float *X, int64_t nn, int64_t d_in, int64_t ldx,
                        const int32_t *y, int64_t n_classes);
int bk_grad_clear(bk_ctx *ctx);
int bk_grad_logistic(bk_ctx *ctx, const double *ww, int where, const int64_t *idx, int64_t count,
                     int64_t batch_size, double alpha, double lammy, const double *noise,
                     int precision, double *delta_out, int64_t *q_out, double *loss_out);
int bk_grad_softmax(bk_ctx *ctx, const double *ww, int where, const int64_t *idx, int64_t count,
                    double max_norm, const double *noise, int precision, double *delta_out,
                    int64_t *q_out, double *loss_out, double *norm_out);
int bk_grad_stats(bk_ctx *ctx, int64_t out[2]);   /* launches, calls so far */

/* Noise application (client DP step) -- requestNoiseFromNoisers
 * (DistSys/main.go:1606-1653: noiseVec = 0 + v_0 + ... + v_{k-1}, then
 * /= float64(k)) and NoisedDelta = Delta + noise (main.go:1524-1537), batched
 * over n updates:
 *     out[i][c] = delta[i][c] + ((0 + noise[i][0][c]) + ... + noise[i][k-1][c]) / k
 * noise vector j of update i starts at d_noise + (i*k + j) * noise_ld.  out may
 * alias delta (out_ld == ld).  k = 0 gives NaN (0/0), as the Go code does. */
int bk_noise_apply_device(bk_ctx *ctx, const double *d_delta, int64_t n, int64_t d, int64_t ld,
                          const double *d_noise, int64_t k, int64_t noise_ld, double *d_out,
                          int64_t out_ld);

/* Noise application fused into the verifier's H2D staging (SURVEY.md §8(f)
 * row 3), then the drop-in Multi-Krum of bk_multikrum on the noised batch.
 * Replaces the host pass NoisedDelta = Delta + noise (main.go:1524-1537,
 * 1606-1653) that precedes getTopKRUMIndex (krum.go:100-166) when the batch is
 * noised where it is verified.  delta: host n x d (row stride ld); noise: host,
 * vector j of update i at noise + (i*k + j) * noise_ld.  Column chunks cross
 * PCIe on a copy stream while K6 noises, and K1 takes the partial Gram of, the
 * previous chunk on the context stream (as bk_multikrum's host path).
 * k = 0 means no noisers: NoisedDelta = Delta (main.go:1599-1602; unlike
 * bk_noise_apply_device, whose k = 0 is the literal 0/0).  where is BK_HOST or
 * BK_HOST_PINNED (pinned memory overlaps; pageable copies are staged by HIP).
 * Outputs as bk_multikrum, plus noised_out (nullable, host n x d, row stride
 * out_ld): the noised batch, bit-identical to bk_noise_apply_device.
 * Synchronous. */
int bk_multikrum_noised(bk_ctx *ctx, const double *delta, int64_t ld, const double *noise,
                        int64_t k, int64_t noise_ld, int where, int64_t n, int64_t d, int64_t f,
                        int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out,
                        double *noised_out, int64_t out_ld);

/* RONI verifier -- roni(ww, delta),
 * ML/code/logistic_validator.py:22-33, batched over n updates:
 *     score[i] = mean(sign(Xv . (ww + delta_i)) != yv) - mean(sign(Xv . ww) != yv)
 * with numpy's sign (0 -> 0, NaN -> NaN, which never equals a label).  Xv is
 * nv x d (row stride ldv), yv the nv labels as doubles (creditcard: -1 / +1,
 * utils.py:96-97), ww d weights, deltas n x d (row stride ld).  The Go verifier
 * rejects an update whose score exceeds 0.02 (main.go:213-226).  Any d
 * (creditcard d = 25), n <= 65534.  Each dot is the fp64 FMA chain over k
 * ascending (on the fp64 MFMA, which rounds exactly so). */
int bk_roni_device(bk_ctx *ctx, const double *d_Xv, int64_t nv, int64_t d, int64_t ldv,
                   const double *d_yv, const double *d_ww, const double *d_deltas, int64_t n,
                   int64_t ld, double *d_scores);
/* The Go verifier's shape: the validation set is uploaded once per context
 * (pyInit imports it with the module, honest.go:204-258), then verifyUpdate
 * (honest.go:598-629) scores host updates against the chain's latest model. */
int bk_roni_set_validation(bk_ctx *ctx, const double *Xv, int64_t nv, int64_t d, int64_t ldv,
                           const double *yv);
int bk_roni(bk_ctx *ctx, const double *ww, const double *deltas, int64_t n, int64_t d, int64_t ld,
            double *scores);

/* The torch-path RONI verifier (the mnist / lfw softmax models) --
 * client_obj.roni(ww, delta), ML/Pytorch/client_obj.py:100-112:
 *     updateModel(ww);         original = getTrainErr()
 *     updateModel(ww + delta); after    = getTrainErr();   score = after - original
 * err(w) = 1 - mean(argmax_c(x W^T + b) == y), with w = [W (n_classes x d_in,
 * row-major), b (n_classes)] (SoftmaxModel, ML/Pytorch/softmax_model.py:7-24;
 * d = n_classes * (d_in + 1): mnist 10 x 785 = 7,850) rounded to fp32 after
 * the fp64 add (torch.FloatTensor), each logit the fp64 sum over k ascending of
 * the exact fp32 products plus the bias, rounded once to fp32; argmax as
 * numpy's (first maximum, NaN wins).  Xv is nv x d_in fp32 (row stride ldv),
 * yv the nv labels (int32).  2 <= n_classes <= 16.
 *
 * WHICH SAMPLES: getTrainErr (ML/Pytorch/client.py:136-144) walks the client's
 * SHUFFLED trainloader (client.py:20, shuffle=True) and returns the error of
 * the LAST mini-batch only (its loop overwrites pred / labels), so the
 * reference scores `original` and `after` on two different random batches of
 * batch_size samples (10 in Biscotti, DistSys/honest.go:47).
 *   bk_roni_softmax_batches*  that semantics: the caller draws the batches (its
 *                             loader's shuffles) and passes, per update j, the
 *                             sample indices idx[(2 j) nb .. + nb) (original,
 *                             model ww) and idx[(2 j + 1) nb ..] (after, model
 *                             ww + delta_j); errors are over nb samples
 *   bk_roni_softmax*          every evaluation over the whole set: the
 *                             reference with batch_size >= nv (one batch)
 *
 * NEAR TIES: torch's CPU sgemm accumulates the logits in fp32 in its own
 * order, so its argmax can differ from this one only on samples whose top two
 * logits lie within that rounding.  near_ties (nullable) receives, per
 * evaluation, the number of samples for which
 *     !( l1 - l2 - u (|l1| + |l2|) > E_a + max_c E_c ),  E_c = g (|x| |w_c| + |b_c|),
 * u = 2^-24, g = gamma_{d_in+1}(u) (1 + 2^-10), or any logit is not finite
 * (l1: the winning logit, class a; l2: the best other).  A score can differ
 * from the reference's only if one of its two evaluations has a near tie, and
 * then by at most (near ties) / (samples).  Layout: bk_roni_softmax* n + 1
 * counts (ww, then each update's model); bk_roni_softmax_batches* 2 n (update
 * j: original, after).  A device-side batch index outside [0, nv) gives that
 * update score NaN and near ties -1 (nothing is read out of range); the host
 * form rejects it with BK_EINVAL. */
int bk_roni_softmax_device(bk_ctx *ctx, const float *d_Xv, int64_t nv, int64_t d_in, int64_t ldv,
                           const int32_t *d_yv, int64_t n_classes, const double *d_ww,
                           const double *d_deltas, int64_t n, int64_t ld, double *d_scores,
                           int32_t *d_near_ties);
int bk_roni_softmax_batches_device(bk_ctx *ctx, const float *d_Xv, int64_t nv, int64_t d_in,
                                   int64_t ldv, const int32_t *d_yv, int64_t n_classes,
                                   const double *d_ww, const double *d_deltas, int64_t n,
                                   int64_t ld, const int64_t *d_idx, int64_t nb, double *d_scores,
                                   int32_t *d_near_ties);
/* The Go verifier's shape (verifyUpdate, honest.go:598-629, bound to the
 * torch module's roni): the validation set (the client's training shard) once
 * per context, then host updates scored against the chain's latest model;
 * synchronous. */
int bk_roni_softmax_set_validation(bk_ctx *ctx, const float *Xv, int64_t nv, int64_t d_in,
                                   int64_t ldv, const int32_t *yv, int64_t n_classes);
int bk_roni_softmax(bk_ctx *ctx, const double *ww, const double *deltas, int64_t n, int64_t ld,
                    double *scores, int32_t *near_ties);
int bk_roni_softmax_batches(bk_ctx *ctx, const double *ww, const double *deltas, int64_t n,
                            int64_t ld, const int64_t *idx, int64_t nb, double *scores,
                            int32_t *near_ties);

/* RONI rounds: the verifier's deployed sequence.  Peer.VerifyUpdateRONI
 * (DistSys/main.go:191-233) scores ONE update per RPC against
 * bc.getLatestGradient(), the same model for every update of an iteration
 * (verifyUpdate, honest.go:598-629).  A round holds that model on the device
 * with its evaluation done, so a score call does the new models' work only.
 *   *_round_begin  needs the matching *_set_validation.  ww (d weights; the
 *                  softmax form's d is the validation set's n_classes *
 *                  (d_in + 1)) is at `where` (BK_HOST, BK_HOST_PINNED or
 *                  BK_DEVICE) and is consumed on return; its evaluation (the
 *                  logistic mismatch count; the softmax correct and near-tie
 *                  counts) runs on asynchronously on the context stream.  The
 *                  round lives until the next begin of its kind or the next
 *                  *_set_validation, which invalidates it.
 *   *_round_score  count >= 1 separately allocated rows of d doubles at `where`
 *                  (bk_collect_add's pointer-table contract: 8-byte aligned, no
 *                  pointer retained on return).  Writes scores[i], and for the
 *                  softmax form near_ties (nullable, 1 + count: the base model,
 *                  then update i at 1 + i).  Synchronous.  Every score and
 *                  near-tie count is bitwise what one bk_roni / bk_roni_softmax
 *                  call on the same ww and rows returns.  Groups of up to
 *                  BK_RONI_ROUND_G updates share one launch (one pass over the
 *                  validation set); a larger count is split into groups.
 * BK_EINVAL: a null pointer, count < 1, a bad where, no validation set, d other
 * than the validation set's, or a score without a live round; BK_ENOTSUP: count
 * beyond bk_roni's / bk_roni_softmax's n.  A refused call leaves the round as it
 * was.  Added without a change of BK_ABI_VERSION (14), as bk_collect_add_noised
 * was. */
#define BK_RONI_ROUND_G 8
int bk_roni_round_begin(bk_ctx *ctx, const double *ww, int64_t d, int where);
int bk_roni_round_score(bk_ctx *ctx, const double *const *deltas, int64_t count, int where,
                        double *scores);
int bk_roni_softmax_round_begin(bk_ctx *ctx, const double *ww, int where);
int bk_roni_softmax_round_score(bk_ctx *ctx, const double *const *deltas, int64_t count, int where,
                                double *scores, int32_t *near_ties);
/* The softmax round in the form the reference scores (r16): client_obj.roni
 * measures `original` and `after` on the shuffled loader's LAST mini-batch each
 * (bk_roni_softmax_batches' semantics; 10 samples in Biscotti), so the deployed
 * mnist verifier's call is this one.
 *   *_round_score_batches  scores against the round begun by
 *                  bk_roni_softmax_round_begin; one live round serves this entry
 *                  and bk_roni_softmax_round_score, in any order.  Rows as for
 *                  *_round_score.  idx is a HOST array in
 *                  bk_roni_softmax_batches' layout, count x 2 x nb: update j
 *                  scores `original` on idx[(2 j) nb ..] and `after` on
 *                  idx[(2 j + 1) nb ..]; any nb >= 1.  Writes scores[j] and
 *                  near_ties (nullable, 2 count: update j's original, after).
 *                  Synchronous.  Every score and near-tie count is bitwise what
 *                  one bk_roni_softmax_batches call on the same ww, rows and idx
 *                  returns.  Only the rows go up (the held model is not uploaded
 *                  or prepared again); groups of up to BK_RONI_ROUND_G updates
 *                  share one launch of 2 ceil(nb / 16) workgroups per update.
 * Checked in this order, before any copy, launch or state change (a refused
 * call leaves the round as it was): BK_EINVAL for a null ctx, deltas, idx or
 * scores, count < 1, nb < 1 or a bad where; BK_EINVAL for no validation set or
 * no live round; BK_ENOTSUP for a count beyond bk_roni_softmax's n; BK_EINVAL
 * for a null row (named); BK_EINVAL for an index outside [0, nv) (the update,
 * the evaluation and the position named).  Added without a change of
 * BK_ABI_VERSION (14). */
int bk_roni_softmax_round_score_batches(bk_ctx *ctx, const double *const *deltas, int64_t count,
                                        int where, const int64_t *idx, int64_t nb, double *scores,
                                        int32_t *near_ties);

/* The convergence check: the new model's error and attack rate.
 * checkConvergence (DistSys/honest.go:141-162) scores the block's model with
 * testModel (honest.go:656-675: train_error / getTestErr) and, for the torch
 * datasets, testAttackRate (honest.go:260-275: get17AttackRate).  A context
 * holds up to BK_EVAL_MAX_SETS resident evaluation sets, indexed 0 .. 3 and
 * separate from RONI's validation sets: no bk_eval* call touches a validation
 * set or a live round.
 *   bk_eval_set_logistic  X nv x d fp64 (row stride ldv), y the nv labels as
 *                  doubles; replaces the slot's set.
 *   bk_eval_set_softmax   X nv x d_in fp32 (row stride ldv), y int32 labels in
 *                  [0, n_classes), 2 <= n_classes <= 16; the model's d is
 *                  n_classes * (d_in + 1) (bk_roni_softmax's layout).
 *   bk_eval_clear  empties a slot.
 *   bk_eval        scores ONE model (d doubles at `where`: BK_HOST,
 *                  BK_HOST_PINNED or BK_DEVICE; consumed on return) on nsets
 *                  resident sets of one kind and of the model's d, in one launch
 *                  and one wait.  For sets[s] it writes err[s], wrong[s] and, if
 *                  non-null, near_ties[s].  Synchronous.
 *   bk_eval_stats  out[0]: launches, out[1]: bk_eval / bk_block_finish_eval
 *                  calls, since bk_create.  A call is one launch: the softmax
 *                  model's preparation is folded into it.
 * The arithmetic is bitwise the base-model evaluation of bk_roni /
 * bk_roni_softmax above.  Logistic: each dot the fp64 FMA chain over k
 * ascending, numpy's sign (0 stays 0, NaN never equals a label), wrong the
 * mismatch count, err = (double)wrong / (double)nv, near_ties 0.  Softmax: ww
 * rounded to fp32, each logit the fp64 k-ascending sum of exact fp32 products
 * plus the bias, rounded once to fp32; argmax takes the first maximum and NaN
 * wins; wrong = nv - correct, err = 1.0 - (double)correct / (double)nv,
 * near_ties by the NEAR TIES rule above.
 * Checked in this order, before any copy or launch: BK_EINVAL for a null ctx,
 * ww, sets, err or wrong, nsets outside [1, BK_EVAL_MAX_SETS], a set index
 * outside [0, BK_EVAL_MAX_SETS) or a bad where; then BK_EINVAL (the set named)
 * for an empty slot, sets of mixed kinds, d other than the set's, or a set
 * named twice.  bk_eval_set_*: BK_EINVAL for a bad set index, nv < 1, d < 1,
 * ldv < d, n_classes < 2, a null pointer, or a label outside [0, n_classes)
 * (the sample named); BK_ENOTSUP for n_classes > 16.  Added without a change
 * of BK_ABI_VERSION (14). */
#define BK_EVAL_MAX_SETS 4
int bk_eval_set_logistic(bk_ctx *ctx, int set, const double *X, int64_t nv, int64_t d, int64_t ldv,
                         const double *y);
int bk_eval_set_softmax(bk_ctx *ctx, int set, const float *X, int64_t nv, int64_t d_in, int64_t ldv,
                        const int32_t *y, int64_t n_classes);
int bk_eval_clear(bk_ctx *ctx, int set);
int bk_eval(bk_ctx *ctx, const double *ww, int64_t d, int where, const int *sets, int nsets,
            double *err, int64_t *wrong, int32_t *near_ties);
int bk_eval_stats(bk_ctx *ctx, int64_t out[2]);
/* bk_block_finish followed by bk_eval of the returned model on `sets`, in one
 * call: every output is bitwise the two-call sequence's.  The model is read
 * from the block's device buffer (it is not uploaded again); where the finish
 * is a device-to-host copy the evaluation is queued behind it and both share
 * one wait (DESIGN.md 5t has the measurement).  bk_block_finish's checks
 * run first, then bk_eval's with the block's d; a refused call leaves the block
 * as it was. */
int bk_block_finish_eval(bk_ctx *ctx, double *global_out, int64_t *qsum_out, double *qsum_float_out,
                         const int *sets, int nsets, double *err, int64_t *wrong, int32_t *near_ties);

/* ---- measurement: per-kernel HIP-event timing on the context stream ------- */
enum bk_kernel_id {
    BK_K_GRAM = 0,     /* K1  fp64-MFMA split-K upper-triangle Gram partials */
    BK_K_REDUCE = 1,   /* K1b fixed-order split-K reduce -> packed upper     */
    BK_K_EXPAND = 2,   /* K2t k_transpose: large n, K2's coalesced row copy  */
    BK_K_SCORES = 3,   /* K2  distance row, bitonic sort, sum ranks 1..k    */
    BK_K_RANK = 4,     /* K3  selection rank + mask                          */
    BK_K_COMPACT = 5,  /* K3b mask -> ascending sel_idx                      */
    BK_K_MEAN = 6,     /* K4  masked mean of the selected rows               */
    BK_K_ALLREDUCE = 7,/* C1  RCCL exchange of the packed Gram               */
    BK_K_SYNTH = 8,
    BK_K_H2D = 9,
    BK_K_D2H = 10,
    BK_K_AGGREGATE = 11, /* K4' block aggregation global += sum (bk_aggregate*) */
    BK_K_QSUM = 12,      /* K5  quantised int64 sum (bk_quantized_sum_device)  */
    BK_K_NOISE = 13,     /* K6  noise application (bk_noise_apply_device, bk_collect_add_noised) */
    BK_K_RONI = 14,      /* K7  RONI counts + scores (bk_roni*)                 */
    BK_K_SMALL = 15,     /* K1..K4 fused in one launch for n <= 128 (k_small)   */
    BK_K_SLICE = 16,     /* K1i8 digit slicing + error bound (BK_F32_I8)        */
    BK_K_SCORE_GATHER = 17, /* C2 RCCL all-gather of the split scores (n >= 2049) */
    /* bk_comm_set_mode 2: from the end of the last Gram piece to the end of
     * the last all-reduce -- the exchange time the overlap left exposed
     * (BK_K_ALLREDUCE is then the span from the first all-reduce's start) */
    BK_K_EXCHANGE_EXPOSED = 18,
    BK_K_RONI_ROUND = 19,    /* k_roni_round_sign: a round's score launches (bk_roni_round_score) */
    BK_K_RONI_ROUND_SM = 20, /* k_roni_round_logits (bk_roni_softmax_round_score)  */
    BK_NUM_KERNELS = 21
};
int bk_timing_enable(bk_ctx *ctx, int on);   /* all kernels; clears accumulated timings */
/* Time only the kernels whose bit (1u << kernel_id) is set: every timed kernel
 * adds two event records to the stream.  Clears accumulated timings. */
int bk_timing_select(bk_ctx *ctx, uint32_t kernel_mask);
int bk_timing_read(bk_ctx *ctx, int kernel_id, double *total_ms, int64_t *count);
/* Record the events of a timed kernel on every `every`-th launch only (1, the
 * default: every launch).  Two event records cost a few us of stream time, as
 * much as config B's whole one-launch step: sampling keeps the timed region's
 * step time honest while the kernel is still timed live.  Clears accumulated
 * timings. */
int bk_timing_stride(bk_ctx *ctx, int every);
const char *bk_kernel_name(int kernel_id);
/* The K1 plan for an aligned fp64 shape: S = workgroup groups (row-block
 * sets, bk_plan.hip), kc = columns per k-block, ntile = 64x64 upper sub-tiles,
 * nwg = workgroups of the launch.  Host-side only; ctx may be NULL. */
int bk_plan(bk_ctx *ctx, int64_t n, int64_t d, int64_t *S, int64_t *kc, int64_t *ntile,
            int64_t *nwg);
/* The same plan with the planner's mode forced (0: v7 interleave, 1: v8
 * round-aligned strides, 2: McNaughton pieces, 3: aligned pieces; -1: the
 * planner's own choice) and its round count (0: the planner's choice).  Every
 * mode computes the same Gram; this entry exists so the planner's coverage
 * check can be exercised for all of them (tests/test_abi.py).  Host-side
 * only; ctx may be NULL.  BK_EHIP if the plan fails its coverage check. */
int bk_plan_mode(bk_ctx *ctx, int64_t n, int64_t d, int mode, int rounds, int64_t *S,
                 int64_t *nwg);

#ifdef __cplusplus
}
#endif
#endif /* BK_H_ */
