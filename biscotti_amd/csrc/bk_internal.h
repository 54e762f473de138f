// bk_internal.h -- what the kernel files (bk_gram, bk_scores, bk_mean, bk_small,
// bk_small_batch, bk_small_ragged, bk_i8, bk_aggregate, bk_roni, bk_collect) and the planner
// (bk_plan) offer the files that implement the C ABI: plans, layouts and
// launchers (and the launchers' shared row-type dispatch).  The context those
// files share among themselves is bk_ctx.h, which the kernels never see.  Not
// installed; the public surface is include/bk.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "bk_synth.h"

namespace bk {

// the packed upper's trailing record (bk_upper_elems): {column count, columns
// accumulated on the fp32 MFMA, absolute Gram error bound of the int8-sliced
// columns (K1i8), 0}; every exchange sums it with the tiles
constexpr int BK_UPPER_TRAIL = 4;

// Probe knobs: timing-only ablations (BK_GRAM_MODE, BK_K2_MODE), planner and
// kernel-shape overrides and debug traces, read only by A/B builds
// (build(extra=["-DBK_PROBES"], out=tools/ab/...)).  The product libbk.so
// never reads them, so no environment variable can make it return a wrong
// result with BK_OK.  Knobs that only pick between
// bit-identical paths (BK_TINY, BK_SMALL, BK_STAGE_CHUNK_BYTES) and the test
// knobs that force a loud failure stay in the product.
#ifdef BK_PROBES
inline const char *probe_env(const char *name) { return getenv(name); }
constexpr bool kProbes = true;
#else
inline const char *probe_env(const char *) { return nullptr; }
constexpr bool kProbes = false;
#endif

// Split-K plan of K1 for one (n, d): T = ceil(n/64) sub-tile rows, ntile =
// T(T+1)/2 upper sub-tiles, S k-pieces of kc columns (multiple of 8), one wave
// per (sub-tile, piece) task, four tasks per 256-thread workgroup.
struct Plan {
    int n = 0, T = 0, ntile = 0, S = 0, nwg = 0;
    int64_t d = 0, kc = 0;
};

// K1 v3 (LDS-shared) plan -- DESIGN.md "K1".  Wave-tasks over the 64x64
// upper sub-tiles: OFF (one off-diagonal sub-tile, 16 MFMA per 4-column
// k-step), PAIR (the two diagonal sub-tiles of a 128-row super-block, upper
// 16x16 blocks only: 2 x 10 MFMA) and DIAG1 (one diagonal sub-tile, 10).  A
// group is <= 8 wave-tasks over <= 6 row-blocks; one 512-thread workgroup (8
// waves, 2 per SIMD) per (group, XCD, slice); see bk_plan.hip.
constexpr int G3_MAXB = 6;    // row-block slots staged per workgroup
constexpr int G3_BK = 16;     // columns per k-block (one LDS stage, 128 B per row)
constexpr int G3_STAGES = 3;  // LDS ring depth (2 k-blocks in flight)
constexpr int G3_BLK = 64 * G3_BK * 8;                     // 8 KiB per block per stage
constexpr int G3_STAGE = G3_MAXB * G3_BLK;                 // 48 KiB
constexpr int G3_LDS = G3_STAGES * G3_STAGE;               // 144 KiB
enum { T_NONE = 0, T_OFF = 1, T_PAIR = 2, T_DIAG1 = 3 };

// The exchange overlapped with the Gram (bk_comm_set_mode 2): ONE Gram launch
// whose workgroups are ordered piece by piece (piece p = launched workgroups
// [start[p], start[p + 1])); every workgroup, at its exit, counts itself into
// cnt[p] after an agent-scope release of its partials, and the communication
// stream waits on the count (hipStreamWaitValue32) before it reduces and
// all-reduces piece p -- so the pieces' exchanges overlap the later pieces'
// compute without a launch boundary (and its tail) between the pieces
struct PieceMarks {
    unsigned *cnt = nullptr;  // device memory: one arrival count per piece (zeroed per call)
    unsigned *sig[8] = {};    // signal memory (hipMallocSignalMemory): piece p done -> 1
    int k = 0;
    int start[9] = {};
    int nowt = 0;             // probe build only (BK_PIECES_NOWT): plain stores -- timing A/B, invalid
};
#ifdef __HIPCC__
// Only the pieces before the last are handed to the communication stream
// (the last is reduced behind the Gram on its own stream): their workgroups
// store their partials write-through (sc1) and count themselves -- the
// guide's write-through hand-off (MI355X_MICROARCH.md, correctness
// boundaries; the form k_small uses): every storing wave drains its sc1
// stores (vmcnt 0), a workgroup barrier, then one lane's relaxed agent-scope
// add on the piece's device counter; the workgroup whose add returns the
// piece's count - 1 saw every other one's drained stores, and raises the
// piece's signal word (one system-scope store) for the communication
// stream's hipStreamWaitValue32.  No release fence (a buffer_wbl2 writes back
// the XCD's whole dirty L2, ~6.5 us), and no per-workgroup atomic on the
// signal word itself: those serialised at ~0.15-0.3 us each and cost
// 0.25-0.3 ms per Gram (r6 A/B, tools/ab_overlap.py).
__device__ inline bool piece_handed(const PieceMarks &pm) {
    return pm.k > 1 && (int)blockIdx.x < pm.start[pm.k - 1];
}
__device__ inline void piece_done(const PieceMarks &pm) {
    if (!piece_handed(pm)) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        int p = 0;
        while (p + 1 < pm.k && (int)blockIdx.x >= pm.start[p + 1]) ++p;
        const unsigned n_p = (unsigned)(pm.start[p + 1] - pm.start[p]);
        if (__hip_atomic_fetch_add(pm.cnt + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
            n_p - 1u)
            __hip_atomic_store(pm.sig[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// a partial's store: write-through (sc1) in a handed-off piece, plain otherwise
__device__ __forceinline__ void st_part(double *p, double v, bool wt) {
    if (wt)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}
#endif

struct GroupDesc {
    int nb;               // row-blocks staged (even; padded with a duplicate)
    int blk[G3_MAXB];     // 64-row block index per slot
    int Q;                // workgroups of this group per XCD
    int wg0;              // offset of this group's list in wglist
    int cost;             // max over SIMDs of its two waves' MFMA units per k-step
    int task[8][5];       // per wave: {kind, slotA, slotB, u0, u1}
    // balanced band quads (bk_plan.hip): block (0,3) of each diagonal tile moves
    // from the PAIR wave to a super-tile OFF wave holding that row-block.
    // xt: PAIR 1 = skip block (0,3); OFF 1 / 2 = also compute block (0,3) of the
    // diagonal tile of its A / B row-block, into slab slot xslot (the PAIR's)
    int xt[8];
    int xslot[8];
};

struct Plan3 {
    int n = 0, T = 0, ntile = 0, ngroups = 0, nwg = 0, nfull = 0;
    int64_t d = 0;
    GroupDesc *d_groups = nullptr;  // device copies (owned by the context)
    int nvwg = 0;                   // virtual workgroups (segments): one partial slab each
    int *d_seg = nullptr;           // per launched workgroup: {first segment, segment count}
    int *d_wg = nullptr;            // per segment: {group, kstart, kstride, kend, tail}
    int *d_red = nullptr;           // per sub-tile u: {list offset, count, slot}
    int *d_wglist = nullptr;        // per group: its workgroups, in reduction order
};

// host planner (bk_plan.hip)
struct Plan3Host {
    int T = 0, ntile = 0, nfull = 0;
    std::vector<GroupDesc> groups;
    std::vector<int> seg;     // 2 per launched workgroup: its segments [v0, v0 + count)
    std::vector<int> wg;      // 5 per segment (a "virtual workgroup": one group, one slab)
    std::vector<int> red;     // 3 per sub-tile
    std::vector<int> wglist;  // concatenated per-group workgroup lists
};
// bk = columns per k-block: 16 for fp64 input, 32 for fp32 (128 B per row either way)
// mode / rounds >= 0 / > 0: force a planner mode (0 v7, 1 v8 strides, 2 McNaughton,
// 3 aligned pieces) and round count (bk_plan_mode); -1 / 0: the planner's choice
Plan3Host build_plan3(int n, int64_t d, int num_cu, int bk = G3_BK, int mode = -1, int rounds = 0);

// K1 v3: one launched workgroup runs its segments one after the other (a CU's
// share of the columns may span two groups: bk_plan.hip "McNaughton")
hipError_t launch_gram3(const void *X, int dtype, int64_t ld, int n, int64_t d, const Plan3 &pl,
                        double *part, hipStream_t st, int mode = 0, long long *trace = nullptr,
                        bool f32_mfma = false, const int *seg = nullptr, int nwg = -1,
                        const PieceMarks &pm = PieceMarks());
// fp32 rows for the fp32-MFMA K1 (a distinct element type selects the kernel)
struct f32m {
    float v;
    __host__ __device__ operator double() const { return v; }
};
// f32_mfma: K1 ran on the fp32 MFMA (the record's second trailing element)
// u0 / u1 / rec: only sub-tiles [u0, u1) (u1 < 0: all), the trailing record
// written only with rec -- one piece of an exchange overlapped with the Gram
hipError_t launch_reduce3(const double *part, const Plan3 &pl, double *U, hipStream_t st,
                          bool f32_mfma, int u0 = 0, int u1 = -1, bool rec = true);
// A split of K1 v3's plan into k launches whose sub-tiles are contiguous
// pieces [tile_end[p - 1], tile_end[p]) of the packed upper (rows of 64-row
// blocks), every launched workgroup's segments inside one piece: the same
// segments and slabs as the one launch, so every sub-tile's sum is bitwise
// the same.  seg: per piece, 2 ints per launched workgroup (as Plan3Host::seg,
// the XCD mapping b = 8 j + x kept).  False (k = 1) when the plan has no such
// split (a workgroup spanning two pieces: the McNaughton plans of n <= 1024)
bool plan3_pieces(const Plan3Host &H, int k, std::vector<int> &tile_end,
                  std::vector<std::vector<int>> &seg);
// the row-block cuts of a k-piece split: weights w[b] of the row blocks,
// valid[b] whether a cut before block b is allowed; the pieces shrink
// geometrically (x0.6) so the last exchange, the one left exposed, is small
std::vector<int> piece_cuts(const std::vector<double> &w, const std::vector<char> &valid, int k);
// the dynamic-LDS limits of the general chain's kernels, file by file
// (bk_gram.hip, bk_scores.hip, bk_mean.hip)
hipError_t configure_gram_kernels();
hipError_t configure_scores_kernels();
hipError_t configure_mean_kernels();
inline hipError_t configure_kernels() {
    hipError_t e = configure_gram_kernels();
    if (e == hipSuccess) e = configure_scores_kernels();
    if (e == hipSuccess) e = configure_mean_kernels();
    return e;
}
// Rows of dtype (0: fp64, else fp32) that can be read as pairs of columns, one
// 16-byte (fp64) or 8-byte (fp32) load each: an even ld and a base aligned to
// a pair.  K1 v1 and K4 pick their VEC kernels by it
inline bool rows_pair_aligned(const void *X, int dtype, int64_t ld) {
    return (ld % 2) == 0 && ((uintptr_t)X % (dtype == 0 ? 16 : 8)) == 0;
}
// (dtype, vec) -> f(T(), std::bool_constant<VEC>()): T = double / float
template <typename F>
inline void with_row_type(int dtype, bool vec, F &&f) {
    if (dtype == 0)
        vec ? f(double(), std::true_type()) : f(double(), std::false_type());
    else
        vec ? f(float(), std::true_type()) : f(float(), std::false_type());
}
hipError_t launch_gram(const void *X, int dtype, int64_t ld, int n, int64_t d, const Plan &pl,
                       double *part, hipStream_t st);
hipError_t launch_reduce(const double *part, const Plan &pl, double *U, hipStream_t st);
hipError_t launch_sum_ranks(const double *Ug, int R, int64_t stride, double *U, hipStream_t st);
hipError_t launch_add_upper(double *U, const double *P, int64_t count, hipStream_t st);
// Ut / dg: nullable (large n: k_transpose's transposed off-diagonal tiles and
// contiguous diagonal, for coalesced row reads)
// r0 / rows: score rows [r0, r0 + rows) only (rows < 0: to n), writing scores[i]
// and diag[i] for those rows (split scoring over the ranks of a sharded call)
hipError_t launch_scores(const double *U, const double *Ut, const double *dg, int T, int n,
                         int64_t k, double *scores, double *diag, hipStream_t st, int r0 = 0,
                         int rows = -1);
bool scores_transposed(int n);
// bj0 / bj1: transpose only the off-diagonal tiles of block-columns bj0..bj1
// (bj1 < 0: all); the diagonal always
hipError_t launch_transpose(const double *U, int T, double *Ut, double *dg, hipStream_t st,
                            int bj0 = 0, int bj1 = -1);
hipError_t launch_rank(const double *scores, int n, int m, int *mask, double *bnd,
                       hipStream_t st);
// split scoring: gathered {ch scores, status} slices -> n contiguous scores,
// and rec = dcols[0..2] (NaN when a rank's status is not 0)
hipError_t launch_split_unpack(const double *sg, int64_t ch, int parts, int n, const double *dcols,
                               double *scores, double *rec, hipStream_t st);
// The device margin record: MARGIN_WORDS doubles, the public 8 (bk.h
// bk_selection_margin_record) then u_G.  margin[2] codes besides 0 / 1 mark
// the call's outputs invalid (read_margin turns them into errors):
constexpr int MARGIN_WORDS = 9;
constexpr double MARGIN_HANDOFF_TIMEOUT = 2.0;  // k_small: a hand-off wait gave up
constexpr double MARGIN_POISONED = 3.0;         // a shard failed before the exchange
constexpr double MARGIN_QUEUE_DIRTY = 4.0;      // k_small (BK_SMALL_CHECK_LINES): a queue word
                                                // other than word 0 of its line was written
// margin: nullable (MARGIN_WORDS doubles, see k_compact); dcols: the packed upper's two
// trailing elements {column count, columns accumulated on the fp32 MFMA}
hipError_t launch_compact(const int *mask, int n, int64_t *sel, const double *diag,
                          const double *bnd, const double *dcols, int64_t k, double *margin,
                          hipStream_t st);
// K4 of a large selection (m >= MEAN_SEG_MIN) sums the selected rows in
// segments of MEAN_SEG_ROWS (seg_part: mean_segments(m) * d doubles), then
// the segments in order; the order depends on m only
constexpr int MEAN_SEG_MIN = 1024, MEAN_SEG_ROWS = 256;
inline int mean_segments(int m) { return m >= MEAN_SEG_MIN ? (m + MEAN_SEG_ROWS - 1) / MEAN_SEG_ROWS : 1; }
hipError_t launch_mean(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *sel, int m,
                       double *mean, int num_cu, hipStream_t st, double *seg_part = nullptr);
// global[c] += X[idx[0]][c] + X[idx[1]][c] + ... (sequential, idx order)
hipError_t launch_accumulate(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *idx,
                             int m, double *global, int num_cu, hipStream_t st);
// bk_aggregate.hip
hipError_t launch_qsum(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *idx, int m,
                       double scale, int64_t *sum, double *sumf, int num_cu, hipStream_t st);
hipError_t launch_noise(const double *delta, int64_t ld, int64_t n, int64_t d, const double *noise,
                        int64_t k, int64_t nld, double *out, int64_t old, int num_cu,
                        hipStream_t st);
hipError_t configure_aggregate_kernels();
// bk_roni.hip
// K7: ws = roni_ws(n, d) bytes (the models' weights, k-major)
size_t roni_ws(int64_t n, int64_t d);
hipError_t launch_roni(const double *Xv, int64_t nv, int64_t d, int64_t ldv, const double *yv,
                       const double *ww, const double *deltas, int64_t n, int64_t ld,
                       double *ws, unsigned int *cnt, double *scores, hipStream_t st);
// the torch-path (softmax model) RONI, K8: ws = roni_softmax_ws(n, din, nv, C) bytes;
// good: 2 (n + 1) counters; xn: the samples' norms (nullable: computed into ws);
// near_out (nullable): the n + 1 near-tie counts (ww, then each update's model)
size_t roni_softmax_ws(int64_t n, int64_t din, int64_t nv, int C);
double roni_softmax_g(int64_t din);
hipError_t launch_roni_xnorm(const float *Xv, int64_t nv, int64_t din, int64_t ldv, double *xn,
                             hipStream_t st);
hipError_t launch_roni_softmax(const float *Xv, int64_t nv, int64_t din, int64_t ldv,
                               const int32_t *yv, int C, const double *ww, const double *deltas,
                               int64_t n, int64_t ld, double *ws, const double *xn,
                               unsigned int *good, double *scores, int32_t *near_out,
                               hipStream_t st);
// K8 on the last mini-batches (idx: n x 2 x nb sample indices; near_out nullable, 2 n)
hipError_t launch_roni_softmax_batches(const float *Xv, int64_t nv, int64_t din, int64_t ldv,
                                       const int32_t *yv, int C, const double *ww,
                                       const double *deltas, int64_t n, int64_t ld,
                                       const int64_t *idx, int64_t nb, double *scores,
                                       int32_t *near_out, hipStream_t st);
// RONI rounds: with n = 0 launch_roni / launch_roni_softmax evaluate ww alone
// (cnt[0]; good[0] and good[1], its near ties) and write no score.  A score
// launch takes up to RONI_ROUND_G new models (rows.p[0..g), d doubles each)
// through one pass over the validation set; cnt: ROUND_CNT_WORDS zeroed words
// of its own; base: the begin's counts; scores (g) and near (softmax, nullable:
// near[0] the base when `first`, near[1 + i] model i) are written by the last
// workgroup out
constexpr int RONI_ROUND_G = 8, ROUND_CNT_WORDS = 32;
struct RoundRows {
    const double *p[RONI_ROUND_G];
};
hipError_t launch_roni_round(const double *Xv, int64_t nv, int64_t d, int64_t ldv, const double *yv,
                             const double *ww, const RoundRows &rows, int g, unsigned int *cnt,
                             const unsigned int *base, double *scores, hipStream_t st);
hipError_t launch_roni_softmax_round(const float *Xv, int64_t nv, int64_t din, int64_t ldv,
                                     const int32_t *yv, int C, const double *ww,
                                     const RoundRows &rows, int g, const double *xn,
                                     unsigned int *cnt, const unsigned int *base, double *scores,
                                     int32_t *near, int first, hipStream_t st);
// The mini-batch form of a softmax round's score launch (k_roni_round_batch):
// up to RONI_ROUND_G updates, each scored as k_roni_batch scores it, on batches
// idx (2 g nb sample indices, range-checked int32: update q's `original` at
// (2 q) nb, its `after` at (2 q + 1) nb) -- idx_dev on the device, or null and
// the indices in idx_arg when there are at most ROUND_IDX_ARGS of them.  cnt:
// ROUND_BATCH_CNT_WORDS zeroed words; scores (g) and near (nullable, 2 g) are
// written by the last workgroup out
constexpr int ROUND_BATCH_CNT_WORDS = 48, ROUND_IDX_ARGS = 256;
struct RoundIdx {
    int32_t v[ROUND_IDX_ARGS];
};
hipError_t launch_roni_softmax_round_batch(const float *Xv, int64_t nv, int64_t din, int64_t ldv,
                                           const int32_t *yv, int C, const double *ww,
                                           const RoundRows &rows, int g, const int32_t *idx_dev,
                                           const RoundIdx &idx_arg, int64_t nb, unsigned int *cnt,
                                           double *scores, int32_t *near, hipStream_t st);
// bk_eval.hip: one model scored on up to EVAL_MAX_SETS resident sets in one
// launch (bk_eval).  A launch's workgroups index the concatenated sample tiles
// of the sets (set i: tiles [tile0, next tile0), EVAL_SIGN_TS / EVAL_LOGITS_TS
// samples each).  cnt: EVAL_CNT_WORDS words, zero before the launch and left
// zero by it ([i]: set i's mismatches / correct predictions, [4 + i]: its near
// ties, [8]: the exit counter); out: the block the last workgroup out writes
constexpr int EVAL_MAX_SETS = 4, EVAL_CNT_WORDS = 16, EVAL_EXIT = 2 * EVAL_MAX_SETS;
constexpr int EVAL_SIGN_TS = 256, EVAL_LOGITS_TS = 64;
struct EvalSet {
    const void *X, *y;  // logistic: doubles; softmax: fp32 samples, int32 labels
    const double *xn;   // softmax: the samples' norms
    int64_t nv, ldv;
    int tile0;
};
struct EvalDesc {
    EvalSet s[EVAL_MAX_SETS];
    int nsets;
};
struct EvalOut {
    double err[EVAL_MAX_SETS];
    int64_t wrong[EVAL_MAX_SETS];
    int32_t near[EVAL_MAX_SETS];
};
hipError_t launch_eval_sign(const EvalDesc &desc, int tiles, const double *ww, int64_t d,
                            unsigned int *cnt, EvalOut *out, hipStream_t st);
hipError_t launch_eval_logits(const EvalDesc &desc, int tiles, const double *ww, int64_t din, int C,
                              unsigned int *cnt, EvalOut *out, hipStream_t st);
// bk_i8.hip: K1i8, the Gram of fp32 rows from exact int8 digit slices
// (BK_F32_I8): column ranges (one per XCD), digit planes [3][npad][dp] int8
struct I8Layout {
    // ns: digit planes (3: the six products of weight >= 2^-26; 2: the three of
    // weight >= 2^-19, BK_F32_I8X2); tj: the output tile's columns (128 / 256)
    int npad = 0, R = 0, T128 = 0, T64 = 0, es = 4, ns = 3, tj = 128;
    int64_t dp = 0, plane = 0, ntile64 = 0;
    std::vector<int64_t> rb;  // range boundaries (R + 1, multiples of 64 columns)
    std::vector<int> order;   // per workgroup {tile I | J << 16, range (-1: idle)}
    std::vector<int> tiles;   // the output tiles (I | J << 16), super-blocked
};
// k pieces of the tile list by 128-row blocks [I0, I1) (the exchange overlapping
// the Gram): per piece its workgroup order (as I8Layout::order) and the
// packed upper's sub-tile range; false when fewer than k cuts exist
bool i8_pieces(const I8Layout &L, int k, std::vector<int> &tile_end,
               std::vector<std::vector<int>> &orders);
I8Layout i8_layout(int n, int64_t d, int es, int num_cu, int ns = 3);
size_t i8_workspace(const I8Layout &L);
hipError_t configure_i8_kernels();
// tables: device copy of {rb (R + 1 int64), order (int pairs)}; ws:
// i8_workspace(L) bytes.  slice: digit planes + the error bound; gemm: the
// range partials; reduce: U (bk_upper_elems(n)) with the trailing record
// {d, 0, bound, 0}
hipError_t launch_i8_slice(const void *X, int dtype, int64_t ld, int n, int64_t d,
                           const I8Layout &L, void *ws, const void *tables, hipStream_t st);
// order / items: one piece's workgroup order (device int pairs), else the layout's
hipError_t launch_i8_gemm(int n, const I8Layout &L, void *ws, const void *tables, hipStream_t st,
                          const void *order = nullptr, int64_t items = -1,
                          const PieceMarks &pm = PieceMarks());
// [e0, e1) elements of U (e1 < 0: all); the record only with rec
hipError_t launch_i8_reduce(int64_t d, const I8Layout &L, void *ws, double *U, hipStream_t st,
                            int64_t e0 = 0, int64_t e1 = -1, bool rec = true);

// bk_small.hip: the whole Multi-Krum of a small batch (n <= 128) in one launch
struct SmallPlan {
    int nb16 = 0, nblk = 0, kc = 0, P = 0, ng = 0, Q = 0, nS = 0, C = 0;  // P chunks, ng G items
};
SmallPlan small_plan(int n, int64_t d, int num_cu);
// n <= 16 and d <= 128 (config A): launch_small runs k_tiny, one workgroup
bool tiny_ok(int n, int64_t d);
constexpr int SMALL_SPLIT_ITEMS = 4;       // G items per chunk (bk_small.hip SMALL_SPLIT)
constexpr int SMALL_CTR_WORDS = 71 * 32;  // 71 queue lines of 128 B (bk_small.hip)
constexpr uint64_t SMALL_SPIN_MAX = 1ull << 24;  // polls before a hand-off wait gives up (~1 s)
hipError_t launch_small(const void *X, int dtype, int64_t ld, int n, int64_t d, int f,
                        const SmallPlan &p, double *part, double *U, double *scores, double *diag,
                        int64_t *sel, double *mean, double *margin, unsigned *ctr, int num_cu,
                        hipStream_t st, long long *trace = nullptr,
                        uint64_t spin_max = SMALL_SPIN_MAX, int check_lines = 0,
                        double *scores_out = nullptr, int g0 = 0, int gn = -1, bool sm = true);
// k_collect_small: the finish of an incremental collection for n <= 128 in one
// launch -- k_small's S and M items on the collection's Gram G (by arrival
// slot, lower packed) and row store, through order (nullable: 0..n-1; it
// travels in the kernel arguments).  sel, mean (nullable), margin and
// scores_out (nullable) may be mapped host memory; scores and diag are device
// scratch of n doubles; ctr: k_small's queue lines
hipError_t launch_collect_small(const void *store, int dtype, int64_t ld, int n, int64_t d, int f,
                                const double *G, const int64_t *order, double *scores,
                                double *diag, int64_t *sel, double *mean, double *margin,
                                double *scores_out, unsigned *ctr, int num_cu, hipStream_t st,
                                uint64_t spin_max = SMALL_SPIN_MAX, int check_lines = 0);
// bk_collect_arrive.hip, k_collect_arrive (bk_collect_add_finish): the border
// of the one new row at arrival slot j <= 127 (already copied into the row
// store; its Gram run is written into G) and k_collect_small's finish behind
// it, in one launch; d <= 32,768 (small_ok).  Every Gram element is the bits
// of k_border + k_border_reduce (bk_collect.hip), whose chunk this is; the
// other arguments are launch_collect_small's
constexpr int COLLECT_BORDER_CHUNK_BYTES = 8192;
hipError_t launch_collect_arrive(const void *store, int dtype, int64_t ld, int j, int n, int64_t d,
                                 int f, double *G, const int64_t *order, double *scores,
                                 double *diag, int64_t *sel, double *mean, double *margin,
                                 double *scores_out, unsigned *ctr, int num_cu, hipStream_t st,
                                 uint64_t spin_max = SMALL_SPIN_MAX, int check_lines = 0);
// bk_collect_arrive_noised.hip, k_collect_arrive_noised
// (bk_collect_add_noised_finish): launch_collect_arrive on an fp64 store with
// the new row noised inside the launch first -- row j = delta + (0 + vecs[0] +
// .. + vecs[k-1]) / k, k_collect_noise's bits.  delta: row j itself (uploaded
// there) or a device row of d doubles, 8-B aligned; vecs: k host-side pointers
// to device vectors of d doubles, 8-B aligned (they travel in the arguments)
constexpr int COLLECT_ARRIVE_NOISE_MAX_K = 64;
hipError_t launch_collect_arrive_noised(const void *store, int64_t ld, int j, const double *delta,
                                        const double *const *vecs, int k, int n, int64_t d, int f,
                                        double *G, const int64_t *order, double *scores,
                                        double *diag, int64_t *sel, double *mean, double *margin,
                                        double *scores_out, unsigned *ctr, int num_cu,
                                        hipStream_t st, uint64_t spin_max = SMALL_SPIN_MAX,
                                        int check_lines = 0);
// bk_collect_tiny.hip, k_collect_tiny (bk_set_collect_tiny): the arrival of cnt
// rows at slots j0.., their border and, with fin, the finish of n rows through
// order, in ONE workgroup; at most COLLECT_TINY_MAX_N rows after the launch, d
// <= COLLECT_TINY_MAX_D.  src[r]: new row r where the device can read it (a row
// of the collection's mapped arrival block, or a device row; d elements, aligned
// to one element).  k > 0 (cnt = 1, fp64): src[0] is the delta and vecs the k
// noise vectors, k_collect_noise's bits.  The store rows and the Gram runs are
// left as bk_collect_add leaves them; sel, mean, margin and scores_out are the
// finish's (launch_collect_small's: the mapped output block)
constexpr int COLLECT_TINY_MAX_N = 16;
constexpr int COLLECT_TINY_MAX_D = 128;
constexpr int COLLECT_TINY_SLOT_BYTES = 1024;  // a row, or a noise vector, of the arrival block
struct CollectTinyLaunch {
    void *store = nullptr;
    int dtype = 0;
    int64_t ld = 0, d = 0;
    double *G = nullptr;
    int j0 = 0, cnt = 0;
    const void *src[COLLECT_TINY_MAX_N] = {};
    const double *const *vecs = nullptr;
    int k = 0;
    int fin = 0, n = 0, f = 0;
    const int64_t *order = nullptr;
    int64_t *sel = nullptr;
    double *mean = nullptr, *margin = nullptr, *scores_out = nullptr;
};
hipError_t launch_collect_tiny(const CollectTinyLaunch &L, hipStream_t st);
// bk_small_batch.hip, k_small_batch / k_tiny_batch: W problems of one shape in one launch (problem
// b's rows at X + b * stride elements).  Per problem: part_stride doubles of
// partials, n scores, n diag, m = n - f sel, d mean (nullable), MARGIN_WORDS of
// margin; lines: (1 + W) * SMALL_CTR_WORDS zeroed queue words (the launch's,
// then each problem's; every launch leaves them zero).  part and lines are
// unused (nullable) when tiny_ok(n, d)
constexpr int SMALL_BATCH_MAX_W = 1024;  // problems per launch (9 KiB of queue lines each)
hipError_t launch_small_batch(const void *X, int dtype, int64_t ld, int64_t stride, int W, int n,
                              int64_t d, int f, const SmallPlan &p, double *part,
                              int64_t part_stride, double *scores, double *diag, int64_t *sel,
                              double *mean, double *margin, unsigned *lines, int num_cu,
                              hipStream_t st, uint64_t spin_max = SMALL_SPIN_MAX);
// bk_small_ragged.hip, k_small_ragged / k_tiny_ragged: W problems in one launch,
// each with its own n and f, all of one NB = ceil(n / 16) and one d (so one P,
// one C, one partials' stride and the instantiation the single call picks: the
// bitwise contract), packed in ONE row-major matrix X.  Problem p of the launch
// is desc[p]: its rows from row `row` of X, its partials in slot `slot` of the
// launch's (part + slot * part_stride), its scores and diag at scores / diag +
// sc, its sel at sel + so, its mean (nullable) at mean + idx * d and its record
// at margin + idx * MARGIN_WORDS -- the caller's positions, so the launches of
// one call fill one set of arrays.  seg: the W + 2 segment starts of the queue
// (ragged_batch_seg_build).  lines: as launch_small_batch's
struct RaggedBatchDesc {
    int32_t n, f, m, idx;  // rows, Byzantine bound, m = n - f; the problem's index in the caller's order
    int64_t row, sc, so;   // offsets: the first row in X, scores / diag, sel
    int32_t slot, pad;     // the problem's partials (and queue lines) in this launch
};
// The queue of k_small_ragged, k_small_batch's lag-one pipeline over W problems
// of NGI G items, n[p] S items and C M items each:
//   G_0 | G_1 S_0 M_0 | G_2 S_1 M_1 | ... | G_{W-1} S_{W-2} M_{W-2} | S_{W-1} M_{W-1}
// segment 0 has NGI items, segment j (1 <= j < W) has NGI + n[j - 1] + C,
// segment W has n[W - 1] + C; seg[0 .. W + 1] are the segments' starts and the
// total.
__host__ __device__ inline void ragged_batch_seg_build(const int32_t *n, int W, int NGI, int C,
                                                       int32_t *seg) {
    seg[0] = 0;
    seg[1] = NGI;
    for (int j = 1; j < W; ++j) seg[j + 1] = seg[j] + NGI + n[j - 1] + C;
    seg[W + 1] = seg[W] + n[W - 1] + C;
}
// queue position item (0 <= item < seg[W + 1]) -> problem p and k_small's item
// number it of that problem (it < NGI: G item it; it < NGI + n[p]: S item
// it - NGI; else M item it - NGI - n[p]).  A binary search over the W + 1
// segments: <= 11 steps at W = 1,024.  A segment's G items open it, and behind
// them the S and M items of the problem before keep k_small's numbering, so no
// n is needed here
__host__ __device__ inline void ragged_batch_queue_decode(const int32_t *seg, int W, int NGI,
                                                          int item, int &p, int &it) {
    int lo = 0, hi = W + 1;  // seg[lo] <= item < seg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= item)
            lo = mid;
        else
            hi = mid;
    }
    const int q = item - seg[lo];
    if (lo == W) {  // the last problem's S and M items
        p = W - 1;
        it = NGI + q;
    } else if (lo == 0 || q < NGI) {  // a G item of the problem that opens the segment
        p = lo;
        it = q;
    } else {  // an S or M item of the problem before
        p = lo - 1;
        it = q;
    }
}
// (the descriptors are the caller's to validate: every n in 16 NB - 15 .. 16 NB,
// 0 <= f < n, m = n - f, slot < W, the offsets inside the arrays; seg =
// ragged_batch_seg_build of the n's with NGI = SMALL_SPLIT_ITEMS * p.P and C =
// p.C (1 without a mean), total = seg[W + 1])
hipError_t launch_small_ragged(const void *X, int dtype, int64_t ld, int W, int NB, int64_t d,
                               const SmallPlan &p, const RaggedBatchDesc *desc, const int32_t *seg,
                               int total, double *part, int64_t part_stride, double *scores,
                               double *diag, int64_t *sel, double *mean, double *margin,
                               unsigned *lines, int num_cu, hipStream_t st,
                               uint64_t spin_max = SMALL_SPIN_MAX);
// k_tiny_ragged: workgroup b is k_tiny on desc[b] (every n <= 16, d <= 128)
hipError_t launch_tiny_ragged(const void *X, int dtype, int64_t ld, int W, int64_t d,
                              const RaggedBatchDesc *desc, double *scores, double *diag,
                              int64_t *sel, double *mean, double *margin, hipStream_t st);
// bk_collect_batch.hip, k_collect_small_batch: W finishes of one shape (n, f)
// over one collection in one launch (problem b's arrival slots at orders +
// b * n).  Per problem: n scores, n diag, m = n - f sel, d mean (nullable),
// MARGIN_WORDS of margin, COLLECT_BATCH_LINES queue lines; lines:
// (COLLECT_BATCH_QLINES + W * COLLECT_BATCH_LINES) * 32 zeroed queue words (the
// launch's, then each problem's; every launch leaves them zero).  W <=
// SMALL_BATCH_MAX_W; the slots are the caller's to validate
constexpr int COLLECT_BATCH_LINES = 13;  // per problem: S arrivals, 8 flag copies, 4 groups
constexpr int COLLECT_BATCH_QLINES = 2;  // per launch: the item head and the error word
hipError_t launch_collect_small_batch(const void *store, int dtype, int64_t ld, int W, int n,
                                      int64_t d, int f, const double *G, const uint16_t *orders,
                                      double *scores, double *diag, int64_t *sel, double *mean,
                                      double *margin, unsigned *lines, int num_cu, hipStream_t st,
                                      uint64_t spin_max = SMALL_SPIN_MAX);
// bk_collect_ragged.hip, k_collect_small_ragged: W finishes over one collection
// in one launch, each with its own n and f, all of one NB = ceil(n / 16) (the
// item bodies pick their summation shapes from NB, and the single finish runs
// the same NB: the bitwise contract).  Problem p of the launch is desc[p]: its
// arrival slots at orders + ord, its scores and diag at scores / diag + sc, its
// sel at sel + so, its mean (nullable) at mean + idx * d and its record at
// margin + idx * MARGIN_WORDS -- the caller's positions, so the launches of one
// call fill one set of arrays.  seg: the W + 2 segment starts of the queue
// (ragged_seg_build).  lines: as launch_collect_small_batch's
struct RaggedDesc {
    int32_t n, f, m, idx;   // rows, Byzantine bound, m = n - f; the problem's index in the caller's order
    int64_t ord, sc, so;    // offsets: the 16-bit slots, scores / diag, sel
};
// The queue of k_collect_small_ragged, a lag-one pipeline over W problems of
// n[p] S items and C M items each:
//   S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}
// segment 0 has n[0] items, segment j (1 <= j < W) has n[j] + C, segment W has
// C; seg[0 .. W + 1] are the segments' starts and the total.
__host__ __device__ inline void ragged_seg_build(const int32_t *n, int W, int C, int32_t *seg) {
    seg[0] = 0;
    seg[1] = n[0];
    for (int j = 1; j < W; ++j) seg[j + 1] = seg[j] + n[j] + C;
    seg[W + 1] = seg[W] + C;
}
// queue position item (0 <= item < seg[W + 1]) -> problem p and k_collect_small's
// item number it of that problem (it < n[p]: S item it; else M item it - n[p]).
// A binary search over the W + 1 segments: <= 11 steps at W = 1,024
__host__ __device__ inline void ragged_queue_decode(const int32_t *seg, int W, int C, int item,
                                                    int &p, int &it) {
    int lo = 0, hi = W + 1;  // seg[lo] <= item < seg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= item)
            lo = mid;
        else
            hi = mid;
    }
    const int q = item - seg[lo];
    // rows of the problem whose S items open segment j (j < W)
    const int nj = lo == 0 ? seg[1] : lo < W ? seg[lo + 1] - seg[lo] - C : 0;
    if (lo < W && q < nj) {
        p = lo;
        it = q;
    } else {  // an M item of the problem before: behind its n[lo - 1] S items
        p = lo - 1;
        it = (lo == 1 ? seg[1] : seg[lo] - seg[lo - 1] - C) + (q - nj);
    }
}
hipError_t launch_collect_small_ragged(const void *store, int dtype, int64_t ld, int W, int NB,
                                       int64_t d, const double *G, const RaggedDesc *desc,
                                       const int32_t *seg, int total, int lead,
                                       const uint16_t *orders, double *scores, double *diag,
                                       int64_t *sel, double *mean, double *margin, unsigned *lines,
                                       int num_cu, hipStream_t st,
                                       uint64_t spin_max = SMALL_SPIN_MAX);
// bk_collect_wide.hip, k_collect_wide / k_collect_wide_ragged: the collection
// finishes for wide rows (n <= 128, d past k_collect_small's cap, opted into by
// bk_set_collect_wide).  k_collect_small's S items and queue with an M item
// that streams: item c owns columns [c W, c W + W), W = COLLECT_WIDE_COLS in
// both dtypes, and adds the m selected rows of the row store in ascending
// order into one fp64 accumulator per column.  The arguments are
// launch_collect_small's and launch_collect_small_ragged's; seg, total and
// lead are built with collect_wide_items(d) M items per problem (1 without a
// mean)
constexpr int COLLECT_WIDE_COLS = 2048;  // columns per M item (a multiple of 64)
inline int collect_wide_items(int64_t d) {
    return (int)((d + COLLECT_WIDE_COLS - 1) / COLLECT_WIDE_COLS);
}
hipError_t launch_collect_wide(const void *store, int dtype, int64_t ld, int n, int64_t d, int f,
                               const double *G, const int64_t *order, double *scores, double *diag,
                               int64_t *sel, double *mean, double *margin, double *scores_out,
                               unsigned *ctr, int num_cu, hipStream_t st,
                               uint64_t spin_max = SMALL_SPIN_MAX, int check_lines = 0);
hipError_t launch_collect_wide_ragged(const void *store, int dtype, int64_t ld, int W, int NB,
                                      int64_t d, const double *G, const RaggedDesc *desc,
                                      const int32_t *seg, int total, int lead,
                                      const uint16_t *orders, double *scores, double *diag,
                                      int64_t *sel, double *mean, double *margin, unsigned *lines,
                                      int num_cu, hipStream_t st,
                                      uint64_t spin_max = SMALL_SPIN_MAX);
// bk_collect_arrive_wide.hip, k_collect_arrive_wide (bk_set_collect_wide_arrive):
// the last arrival of a WIDE row at slot j <= 127 and k_collect_wide's finish
// behind it, in one launch.  The queue numbers four kinds of item in dependency
// order; an item waits only for items numbered before it:
//   B  nB = S RB   chunk s of the new row against the resident rows of block rb
//                  (rpb rows, one per wave and round): k_border's partials for
//                  C = 1 -> P[s (j + 1) + i]
//   R  nR          the chunk sum of WIDE_ARRIVE_NW elements i <= j, one wave
//                  each: k_border_reduce's -> G[j (j + 1) / 2 + i]
//   S  n           k_collect_wide's S items (run j of G read with sc1 loads)
//   M  nM          k_collect_wide's M items (1 without a mean)
// The B items arrive on G_GRP's 32 groups of 32, so nB <= 1,024: rpb is the
// smallest multiple of the workgroup's waves that keeps S ceil(rows / rpb)
// there -- the most items the lines count, for the grid's balance.
constexpr int WIDE_ARRIVE_NW = 8;        // waves of a workgroup (SMALL_NW)
constexpr int WIDE_ARRIVE_MAX_B = 1024;  // B items a launch may number
enum { WIDE_ARRIVE_B = 0, WIDE_ARRIVE_R = 1, WIDE_ARRIVE_S = 2, WIDE_ARRIVE_M = 3 };
struct WideArriveQueue {
    int S, rpb, RB;       // chunks of a row; resident rows per B item; row blocks
    int nB, nR, nS, nM;   // items of each kind, in queue order
};
// rows: the rows collected after the add (j + 1); false outside the range
__host__ __device__ inline bool wide_arrive_queue(WideArriveQueue &q, int64_t rows, int64_t d,
                                                  int dtype, int64_t n, bool mean) {
    if (rows < 1 || rows > 128 || n < 1 || n > 128 || d < 1 || (dtype != 0 && dtype != 1))
        return false;
    const int64_t S = (d * (dtype == 0 ? 8 : 4) + COLLECT_BORDER_CHUNK_BYTES - 1) /
                      COLLECT_BORDER_CHUNK_BYTES;
    if (S > WIDE_ARRIVE_MAX_B) return false;
    int rpb = WIDE_ARRIVE_NW;
    while (S * ((rows + rpb - 1) / rpb) > WIDE_ARRIVE_MAX_B) rpb += WIDE_ARRIVE_NW;
    q.S = (int)S;
    q.rpb = rpb;
    q.RB = (int)((rows + rpb - 1) / rpb);
    q.nB = q.S * q.RB;
    q.nR = (int)((rows + WIDE_ARRIVE_NW - 1) / WIDE_ARRIVE_NW);
    q.nS = (int)n;
    q.nM = mean ? (int)((d + COLLECT_WIDE_COLS - 1) / COLLECT_WIDE_COLS) : 1;
    return true;
}
// item it of the queue -> its kind and (B: chunk a, row block b; R: first
// element a, elements b; S: row a; M: mean item a).  Consecutive B items take
// consecutive chunks of one row block: the workgroups that start together
// stream neighbouring columns of the same rows
__host__ __device__ inline void wide_arrive_decode(const WideArriveQueue &q, int rows, int it,
                                                   int &kind, int &a, int &b) {
    b = 0;
    if (it < q.nB) {
        kind = WIDE_ARRIVE_B;
        a = it % q.S;
        b = it / q.S;
    } else if (it < q.nB + q.nR) {
        kind = WIDE_ARRIVE_R;
        a = (it - q.nB) * WIDE_ARRIVE_NW;
        b = rows - a < WIDE_ARRIVE_NW ? rows - a : WIDE_ARRIVE_NW;
    } else if (it < q.nB + q.nR + q.nS) {
        kind = WIDE_ARRIVE_S;
        a = it - q.nB - q.nR;
    } else {
        kind = WIDE_ARRIVE_M;
        a = it - q.nB - q.nR - q.nS;
    }
}
// P: the collection's partials buffer, S (j + 1) doubles at least; the other
// arguments are launch_collect_arrive's
hipError_t launch_collect_arrive_wide(const void *store, int dtype, int64_t ld, int j, int n,
                                      int64_t d, int f, double *G, double *P, const int64_t *order,
                                      double *scores, double *diag, int64_t *sel, double *mean,
                                      double *margin, double *scores_out, unsigned *ctr, int num_cu,
                                      hipStream_t st, uint64_t spin_max = SMALL_SPIN_MAX,
                                      int check_lines = 0);
hipError_t launch_synth(void *X, int dtype, int64_t ld, int64_t n, int64_t dl, int64_t c0,
                        const int64_t *perm, const SynthParams &P, hipStream_t st);
// bk_collect_noise.hip, k_collect_noise (bk_collect_add_noised): one launch adds
// the mean of its k noise vectors to each of `rows` arriving fp64 rows over the
// columns [c0, c1) (c0 even; c1 even or d), K6's arithmetic: out[r][c] =
// delta[r][c] + ((0 + v_0[c]) + ... + v_{k-1}[c]) / k, k >= 1.  delta[r] may be
// out[r] (in place).  Row r's vector j is tab[r k + j] (tab in device memory:
// the caller's device rows, 8-B aligned at least), or, with tab null, lies in
// the staging block at stage + (r k + j) sld, its column c at [c - c0] (stage
// 16-B aligned, sld even).  out[r] is 16-B aligned; only columns [c0, c1) of
// it are written.  The tables travel in the kernel's arguments
constexpr int COLLECT_NOISE_ROWS = 8;  // rows per launch: k_border's group (BORDER_ROWS)
struct CollectNoiseArgs {
    const double *delta[COLLECT_NOISE_ROWS];
    double *out[COLLECT_NOISE_ROWS];
    const double *const *tab;
    const double *stage;
    int64_t sld, c0, c1;
    int rows, k;
};
hipError_t launch_collect_noise(const CollectNoiseArgs &a, int num_cu, hipStream_t st);

// bk_collect.hip: the incremental collection of a context (bk_collect_*), which
// owns its buffers; bk_destroy frees it (device selected, streams idle)
struct Collect;
void collect_destroy(Collect *k);

// bk_block.hip: one launch group of the miner's block (bk_block_*): up to
// BLOCK_GROUP arrivals added to the running gradient in arrival order,
// gout = gin + rows (another buffer than gin); qin non-null: the quantised
// int64 sum as well, qout = qin + int64(rows * scale); fin: the results also
// stored to the mapped host block hg (and hq, hqf with qin).  rows.p[i] is read
// only where bit i of acc is set; rows aligned to their element size
constexpr int BLOCK_GROUP = 8;
struct BlockRows {
    const void *p[BLOCK_GROUP];
};
struct BlockLaunch {
    BlockRows rows;
    unsigned acc;
    int dtype;
    int64_t d;
    const double *gin;
    double *gout;
    const int64_t *qin;
    int64_t *qout;
    double scale;
    int fin;
    double *hg;
    int64_t *hq;
    double *hqf;
};
hipError_t launch_block_add(const BlockLaunch &L, int num_cu, hipStream_t st);
// bk_block_api.hip: a context's block, which owns its buffers; bk_destroy frees it
struct Block;
void block_destroy(Block *b);

// bk_shares.hip: the secure-aggregation share arithmetic (bk_shares_*,
// DESIGN.md §5u).  Parts and y are [chunk][share] int64; share s sits at
// x = s - SHARES_X0.  Every pointer is device memory, 8-byte aligned
constexpr int SHARES_MAX_POLY = 10;
constexpr int SHARES_MAX_POINTS = 64;
constexpr int SHARES_X0 = 10;
// y[chunk][s], s < T, from the delta's d entries; per_chunk: one thread per
// chunk looping over the shares, else one thread per (chunk, share)
hipError_t launch_shares_gen(const double *delta, int64_t d, double scale, int P, int T,
                             int64_t *y, bool per_chunk, hipStream_t st);
// out[e] = sum_r store[slots[r] * stride + e], e < elems (wrapping); stride
// even, store and out 16-byte aligned
hipError_t launch_shares_sum(const int64_t *store, int64_t stride, int64_t elems,
                             const int64_t *slots, int64_t count, int64_t *out, int num_cu,
                             hipStream_t st);
// point s of chunk c is base[s][c * stride[s]] at node x[s]
struct SharesPoints {
    const int64_t *base[SHARES_MAX_POINTS];
    int stride[SHARES_MAX_POINTS];
    int x[SHARES_MAX_POINTS];
};
// coef / delta nullable; *bad (zeroed by the caller) counts the bad chunks
hipError_t launch_shares_recover(const SharesPoints &pts, int S, int P, int64_t d, double scale,
                                 const double *w, int64_t *coef, double *delta, double *global,
                                 unsigned long long *bad, hipStream_t st);
// bk_shares_api.hip: a context's share state, which owns its buffers
struct Shares;
void shares_destroy(Shares *s);

}  // namespace bk
