// bk_ctx.h -- the context behind the C ABI (struct bk_ctx) and what its entry
// families share: the error string, the status macros, the staging of K1..K4
// and the guards.  Private to the files that implement include/bk.h (bk_api,
// bk_stage, bk_host, bk_comm, bk_group, bk_entries, bk_batch and the host half of
// bk_collect); the kernels see bk_internal.h only.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bk.h"
#include "bk_internal.h"

namespace bk {

class HostPool;  // bk_hostpool.h

// bk_last_error()'s text, per thread (bk_api.hip)
extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(_e == hipErrorOutOfMemory ? BK_ENOMEM : BK_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                \
    } while (0)

#define RCCLCHK(expr)                                                                        \
    do {                                                                                     \
        ncclResult_t _r = (expr);                                                            \
        if (_r != ncclSuccess)                                                               \
            return fail(BK_ERCCL, "%s: %s (%s:%d)", #expr, ncclGetErrorString(_r), __FILE__, \
                        __LINE__);                                                           \
    } while (0)

#define CHK(expr)              \
    do {                       \
        int _s = (expr);       \
        if (_s != BK_OK) return _s; \
    } while (0)

extern const char *kKernelNames[BK_NUM_KERNELS];

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    uint64_t *epoch = nullptr;  // the owning context's ws_epoch (graph invalidation)
};

// A K1 plan's (or K1i8 layout's) split into k launches whose sub-tiles are
// contiguous pieces of the packed upper, for the exchange overlapped with
// the Gram (bk_comm_set_mode 2): piece p's elements are U[e[p], e[p + 1]),
// the last piece's range ending with the trailing record
struct Pieces {
    int k = 0;                // pieces built for (0: none yet)
    bool ok = false;          // false: the plan has no k-piece split
    std::vector<int64_t> e;   // k + 1 element bounds of U
    std::vector<int> nwg;     // per piece: launched workgroups (K1 v3) / items (K1i8)
    std::vector<size_t> off;  // per piece: its table's offset in d (ints)
    int *d = nullptr;         // device copy of the tables, concatenated
};

inline void free_pieces(Pieces &pc) {
    if (pc.d) (void)hipFree(pc.d);
    pc = Pieces();
}

// bk_block_*: the block of a context.  The running gradient
// and the quantised sum are kept twice: a launch group reads g[cur] / q[cur]
// and writes the other pair, and cur flips once the launch is queued, so a
// launch that fails leaves the block as it was.  All buffers grow only.
constexpr int BLOCK_RING_SLOTS = 4;
constexpr size_t BLOCK_RING_SLOT_BYTES = (size_t)1 << 20;
constexpr int BLOCK_ARRIVE_GROUPS = 8;
// The measured cuts (profiles/r20/block_bench.json), in bytes of
// one row / of the gradient; 0: the path is not taken.  Host rows up to
// BLOCK_MAPPED_* are read by the kernel from the mapped arrival block instead
// of being copied to the device; a gradient up to BLOCK_FIN_MAX is stored by
// the kernel into mapped host memory instead of being copied back.  Measured at
// d = 25 .. 262,144 fp64: the mapped rows won through d = 32,768 (21.5 us
// against 34.2 .. 36.0 for add + wait) and lost at 262,144 (108 against 74 ..
// 103); the mapped output won through d = 784 (14.0 against 23.8) and lost from
// 7,850 on (16.4 against 13.2)
constexpr int64_t BLOCK_MAPPED_HOST_MAX = 32768 * 8;
constexpr int64_t BLOCK_MAPPED_PINNED_MAX = 32768 * 8;
constexpr int64_t BLOCK_FIN_MAX = 784 * 8;
struct Block {
    bool begun = false;
    int dtype = BK_F64;
    int64_t d = 0;
    int precision = -1;
    double scale = 1.0;  // 10^precision
    int64_t added = 0, accepted = 0;
    // bk_block_stats, since the begin: add launches, fused add-finish launches,
    // launches that read their rows from mapped host memory, finishes served
    // without a D2H copy call
    int64_t stats[4] = {0, 0, 0, 0};
    double *g[2] = {nullptr, nullptr};
    int64_t *q[2] = {nullptr, nullptr};
    size_t g_elems = 0, q_elems = 0;
    int cur = 0;
    // host rows of one launch group on the device
    char *stage = nullptr;
    size_t stage_bytes = 0;
    // pageable rows go up through this pinned ring, a slot's host copy under
    // the DMA of the one before (the collection's upload_pageable)
    char *ring = nullptr;
    hipEvent_t ev_slot[BLOCK_RING_SLOTS] = {};
    bool slot_used[BLOCK_RING_SLOTS] = {};
    int ring_next = 0;
    hipEvent_t ev_up = nullptr;  // behind a call's copies or launches: its rows are consumed
    // the mapped pinned arrival block small host rows are memcpy'd into and the
    // kernel reads over PCIe (no copy call), BLOCK_GROUP rows of arrive_row bytes
    // A launch group takes the next of BLOCK_ARRIVE_GROUPS group slots and
    // records the slot's event behind its launch; the group that comes round
    // to the slot again waits for that event before the CPU writes
    char *arrive = nullptr, *arrive_dev = nullptr;
    size_t arrive_row = 0;
    hipEvent_t ev_arrive[BLOCK_ARRIVE_GROUPS] = {};
    bool arrive_used[BLOCK_ARRIVE_GROUPS] = {};
    int arrive_next = 0;
    // the mapped pinned output block a FIN launch stores into: d doubles of the
    // gradient, then d int64 and d doubles of the quantised sum; out_valid: it
    // holds the block's current state (no add since the launch that wrote it)
    char *out = nullptr, *out_dev = nullptr;
    size_t out_elems = 0;
    bool out_valid = false;
};

// bk_shares_*: the secure-aggregation share state of a context (DESIGN.md
// §5u).  store: n_cap parts of `stride` int64 each (part_elems = chunks * held
// of them used, stride the next even number: every part starts on 16 bytes);
// own: the last bk_shares_sum's aggregate.  The other buffers stage one call's
// host inputs and outputs.  All grow only
struct Shares {
    bool begun = false;
    int64_t d = 0, chunks = 0, n_cap = 0, count = 0, part_elems = 0, stride = 0;
    int poly = 0, held = 0;
    bool own_valid = false;
    DevBuf store, own, slots, in, w, out, bad;
    // bk_shares_stats, since the context was made: launches, copy calls,
    // calls that reached the device, bad chunks
    int64_t stats[4] = {0, 0, 0, 0};
};

// bk_eval*: the evaluation sets of a context (bk_eval.hip),
// buffers of their own: RONI's validation sets and rounds never see them
enum { EVAL_EMPTY = 0, EVAL_LOGISTIC = 1, EVAL_SOFTMAX = 2 };
struct EvalSlot {
    int kind = EVAL_EMPTY;
    int64_t nv = 0, d = 0;    // samples; the model's length
    int64_t din = 0, C = 0;   // softmax: d = C (din + 1)
    DevBuf X, y, xn;          // compact rows (row stride d / din); xn: softmax only
};
struct Eval {
    EvalSlot set[EVAL_MAX_SETS];
    DevBuf w, cnt;            // a host model's device copy; the launch's counters
    EvalOut *out = nullptr, *out_dev = nullptr;  // mapped pinned: the last workgroup's stores
    int64_t launches = 0, calls = 0;             // bk_eval_stats
};

// bk_grad*: the peer's resident training shard and the scratch of one gradient
// step (bk_grad_api.hip, kernels bk_grad.hip), buffers of their
// own: the eval sets, RONI's validation sets and live rounds never see them.
// All grow only
constexpr int GRAD_TILE = 256;             // batch positions per chain
constexpr int64_t GRAD_MAX_BATCH = 65536;  // rows of one step
constexpr int64_t GRAD_MAX_D = 32768;      // logistic d, softmax d_in
constexpr int64_t GRAD_MAPPED_MAX = 784;   // host outputs up to here are stored into mapped memory
struct GradOut {                           // the mapped block's head
    double loss, norm;
};
struct Grad {
    int kind = EVAL_EMPTY;    // EVAL_LOGISTIC / EVAL_SOFTMAX
    int64_t nn = 0, d = 0;    // rows; the model's length
    int64_t din = 0, C = 0;   // softmax: d = C (din + 1)
    DevBuf X, y;              // compact rows (row stride d / din)
    DevBuf w, noise, idx;     // a call's host inputs on the device
    DevBuf R;                 // softmax: the batch's residuals, positions x 16
    DevBuf part, lossp;       // per-tile partial sums; per-workgroup loss parts
    DevBuf out;               // host outputs beyond GRAD_MAPPED_MAX: d doubles, then d int64
    DevBuf cnt;               // the exit counter (zeroed once: every launch leaves it zero)
    // mapped pinned: GradOut, then GRAD_MAPPED_MAX doubles and as many int64
    char *hout = nullptr, *hout_dev = nullptr;
    int64_t launches = 0, calls = 0;  // bk_grad_stats
};
void grad_destroy(Grad *g);
// bk_grad.hip.  rows: the batch's row numbers on the device (null: 0 .. count-1);
// noise / q nullable; out: the mapped GradOut's device address.  part holds
// tiles x d doubles (logistic: only with more than one tile), lossp one double
// per workgroup of the (forward) launch, cnt one zeroed word
struct GradLogistic {
    const double *X, *y, *ww, *noise;
    const int64_t *rows;
    int64_t count, d;
    double batch, alpha, lammy, scale;
    double *part, *lossp, *delta;
    int64_t *q;
    GradOut *out;
    unsigned int *cnt;
};
hipError_t launch_grad_logistic(const GradLogistic &a, hipStream_t st);
struct GradSoftmax {
    const float *X;
    const int32_t *y;
    const double *ww, *noise;
    const int64_t *rows;
    int64_t count, din;
    int C;
    double max_norm, scale;
    double *R, *part, *lossp, *delta;
    int64_t *q;
    GradOut *out;
    unsigned int *cnt;
};
hipError_t launch_grad_softmax_fwd(const GradSoftmax &a, hipStream_t st);
hipError_t launch_grad_softmax_bwd(const GradSoftmax &a, hipStream_t st);

// bk_commit_*: the resident commitment key of a context and a call's scratch
// (bk_commit_api.hip, kernels bk_commit.hip).  table: per key
// point its multiples 1 .. 8, affine, in Montgomery form (512 bytes); replaced
// only by a bk_commit_set_key that succeeds.  The other buffers grow only
constexpr int64_t COMMIT_MAX_KEY = (int64_t)1 << 22;  // key points (a 2 GiB table)
constexpr int COMMIT_MAX_GROUPS = 256;                // workgroups of one k_commit_msm
constexpr int COMMIT_MSM_TERMS = 4;                   // terms per thread it aims at
struct Commit {
    uint32_t *table = nullptr;
    int64_t count = 0;
    DevBuf in, out;    // a call's host scalars / delta and outputs on the device
    DevBuf part, cnt;  // the workgroups' sums; the exit counter (zeroed once: every launch leaves it zero)
    DevBuf bad;        // set_key: the smallest invalid index
    // bk_commit_stats: launches, copy calls, calls that reached the device
    int64_t stats[3] = {0, 0, 0};
    // the terms per thread k_commit_msm's grid aims at (BK_COMMIT_MSM_TERMS, read
    // when the state is made, for tools/commit_bench.py; the same bytes)
    int terms = COMMIT_MSM_TERMS;
};
void commit_destroy(Commit *cm);
// bk_commit.hip.  Every pointer is device memory.  Exactly one of delta / q is
// non-null: the scalars are q, or int64(delta * scale) by Go's conversion.
// table points at the first key point's entry.  pk: count x 64 bytes, 4-byte
// aligned; *bad (preset to all ones) takes the smallest invalid index
hipError_t launch_commit_key(const uint8_t *pk, int64_t count, uint32_t *table,
                             unsigned long long *bad, hipStream_t st);
// part: commit_msm_groups(n, terms) x 24 words; cnt one zeroed word; out 64 bytes
int commit_msm_groups(int64_t n, int terms);
hipError_t launch_commit_msm(const double *delta, const int64_t *q, double scale, int64_t n,
                             const uint32_t *table, uint32_t *part, unsigned int *cnt,
                             uint8_t *out, int terms, hipStream_t st);
// out: chunks x 64 bytes / chunks x T x 64 bytes, chunks = ceil(d / P)
hipError_t launch_commit_chunks(const double *delta, const int64_t *q, double scale, int64_t d,
                                int P, const uint32_t *table, uint8_t *out, hipStream_t st);
hipError_t launch_commit_witness(const double *delta, const int64_t *q, double scale, int64_t d,
                                 int P, int T, const uint32_t *table, uint8_t *out,
                                 hipStream_t st);

}  // namespace bk

// the C ABI's opaque handle, hence at global scope; its field types are bk::'s
using namespace bk;

struct bk_ctx {
    int device = 0;
    int num_cu = 256;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // workspace (grow-only)
    DevBuf part, U, Ug, scores, mask, sel, X, mean, perm, trace, idx;
    // the selection margin of the last finish (K2 diag, K3 boundary scores, K3b record)
    DevBuf diag, bnd;
    DevBuf Ut;  // K2 at large n: transposed off-diagonal tiles + diagonal (k_transpose)
    // k_small (n <= 128, one launch): its queue counters (zeroed once; every
    // launch leaves them zero) and the split-K partials
    DevBuf small_ctr, small_part;
    // bk_multikrum_batch*: buffers of their own (a single call or a collection
    // finish between two batched calls is unaffected): the queue lines (the
    // launch's, then one set per problem; zeroed at allocation, every launch
    // leaves them zero), the partials of one launch, per-problem diag and
    // scratch scores, the batch x MARGIN_WORDS records, and the host entry's
    // device copies of X and of the outputs
    DevBuf batch_ctr, batch_part, batch_diag, batch_scores, batch_rec;
    DevBuf batch_X, batch_sel, batch_hsc, batch_mean;
    // bk_multikrum_ragged*: a call's descriptors and segment starts on the
    // device, and the pinned ring they go up through -- a call fills the next
    // slot and records the slot's event behind its copy, and the call that
    // comes round to the slot again waits for that event before it writes, so
    // calls queued back to back on the stream never share staging bytes
    DevBuf batch_desc;
    static constexpr int RAGGED_SLOTS = 4;
    void *ragged_stage[RAGGED_SLOTS] = {};
    size_t ragged_stage_bytes[RAGGED_SLOTS] = {};
    hipEvent_t ev_ragged[RAGGED_SLOTS] = {};
    bool ragged_used[RAGGED_SLOTS] = {};
    int ragged_next = 0;
    // the records of the last batched call on the host (fetched by the first
    // reader once the stream is done) and the one bk_selection_margin* reports
    // (margin_host points at batch_pick while a batched call is the last finish)
    std::vector<double> batch_rec_h;
    int64_t batch_last = 0;   // problems of the last batched call
    int batch_fetched = 0;
    int batch_one = 0;        // the last batched call had one problem: the single call's own record
    double batch_pick[MARGIN_WORDS] = {0};
    DevBuf mean_part;  // K4 of a large selection: per-segment column sums (launch_mean)
    int small_on = 1;
    int collect_wide = 0;  // bk_set_collect_wide: the wide one-launch collection finishes (opt-in)
    int collect_tiny = 0;  // bk_set_collect_tiny: the one-workgroup tiny collection (opt-in)
    int collect_wide_arrive = 0;  // bk_set_collect_wide_arrive: the fused wide last arrival (opt-in)
    uint64_t small_spin_max = SMALL_SPIN_MAX;  // test knob BK_SMALL_SPIN_MAX=<polls>[,<launches>]
    int64_t small_spin_left = -1;              // ... for this many launches (-1: all)
    int small_check_lines = 0;                 // debug knob BK_SMALL_CHECK_LINES (bk_create)
    int margin_valid = 0;
    // a finish ran since its record's error codes were last read (bk_synchronize
    // reads them: an asynchronous caller learns of an invalid call there)
    int margin_unchecked = 0;
    int64_t spin_us = 2000;  // wait_stream: poll this long before blocking (BK_SPIN_US)
    // the record of the last finish, written by the kernels straight into mapped
    // pinned memory (GPU-cached, written back at the kernel's end): the host
    // reads it after the stream has finished, with no device-to-host copy
    double *hmargin = nullptr;
    double *dmargin = nullptr;  // its device address
    // pinned: the n <= 128 host entries' outputs {margin, sel, scores, mean},
    // read back in one copy (a D2H into pageable memory goes through HIP's
    // staging: ~20 us per copy at config B)
    void *hout = nullptr;  // the host small path's mapped output block (pinned)
    size_t hout_bytes = 0;
    double *hout_dev = nullptr;          // its device address
    const double *hout_host_margin = nullptr;  // its record, as the host reads it
    const double *margin_host = nullptr;  // non-null: the last call's record is there
    // BK_F32_CERTIFIED: 1 while the exact re-run of a near-tie call is in progress
    int force_exact = 0;
    int64_t certified_reruns = 0;
    // RONI: the validation set (bk_roni_set_validation) and per-call scratch
    DevBuf roni_X, roni_y, roni_w, roni_d, roni_cnt, roni_s;
    int64_t roni_nv = 0, roni_dim = 0;
    // the torch-path (softmax) RONI: its validation set (fp32 samples, int32
    // labels; bk_roni_softmax_set_validation) and the prepared models
    DevBuf rmc_X, rmc_y, rmc_ws, rmc_xn, rmc_idx, rmc_nt;
    int64_t rmc_nv = 0, rmc_din = 0, rmc_C = 0;
    // RONI rounds (bk_roni*_round_*): the iteration's model, its evaluation's
    // counts (logistic: mismatches; softmax: correct, near ties) and the begin's
    // prepared columns (softmax: the widened fp32 weights and their norms), kept
    // until the next begin or set_validation; buffers of their own, so batched
    // calls in between leave a round intact
    DevBuf rr_w, rr_base, rr_ws, rs_w, rs_base, rs_ws;
    int rr_live = 0, rs_live = 0;
    // a score call's scratch: host rows staged on the device, the groups'
    // counters, and the mapped pinned block the kernel writes the scores (and
    // near-tie counts) into: no device-to-host copy; round_idx: the mini-batch
    // form's sample indices when a group has too many for the kernel's
    // arguments (they go up through the ragged calls' pinned ring)
    DevBuf round_rows, round_cnt, round_idx;
    void *round_out = nullptr;
    void *round_out_dev = nullptr;
    size_t round_out_bytes = 0;
    hipEvent_t ev_round = nullptr;  // begin: ww has been consumed
    // bk_multikrum_noised: a 2-slot ring of noise chunks, filled on a copy
    // stream while K6 consumes the previous chunk on `stream` (created lazily)
    DevBuf noise;
    hipStream_t copy = nullptr;
    hipEvent_t ev_go = nullptr, ev_cp[2] = {nullptr, nullptr}, ev_use[2] = {nullptr, nullptr};
    // host-side pinned allocations handed out by bk_stage_alloc
    std::vector<void *> staged;
    // bk_multikrum_rows: worker threads packing the caller's separate host rows
    // into a pinned ring (both created on first use), and the ring slots'
    // copy-done events
    bk::HostPool *hpool = nullptr;
    int hthreads = 0;  // packing threads incl. the caller (bk_set_host_threads; 0: default)
    void *rstage = nullptr;
    size_t rstage_bytes = 0;
    hipEvent_t ev_rows[4] = {nullptr, nullptr, nullptr, nullptr};
    // timing
    uint32_t timing = 0;  // bit k: record HIP events around kernel k (bk_timing_select)
    int tstride = 1;      // ... on every tstride-th launch of it (bk_timing_stride)
    int64_t tseq[BK_NUM_KERNELS] = {0};
    struct Ev {
        int kid;
        hipEvent_t a, b;
    };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    double tot_ms[BK_NUM_KERNELS] = {0};
    int64_t cnt[BK_NUM_KERNELS] = {0};
    // K1 v3 plans (device tables), cached per (n, d)
    struct CachedPlan {
        int n;
        int64_t d;
        int bk;  // columns per k-block (16 fp64, 32 fp32)
        Plan3 p;
        Pieces pc;
    };
    std::vector<CachedPlan> plans;
    // K1i8 (BK_F32_I8): layouts and device tables per (n, d), and the workspace
    struct I8Cached {
        int64_t n = 0, d = 0;
        I8Layout L;
        void *tables = nullptr;
        Pieces pc;
    };
    std::vector<I8Cached> i8;
    DevBuf i8ws;
    // K1i8 signatures {n, d, element size, digits} whose workspace failed to
    // allocate: they run exact until the mode is set again (bk_set_f*_mode)
    std::vector<std::array<int64_t, 4>> i8_failed;
    int gram_variant = 3;  // 3: LDS-shared v3 for aligned fp64; 1: v1 everywhere (BK_GRAM=v1)
    int gram_mode = 0;     // BK_GRAM_MODE: timing-only ablations of v3 (tools/, never tests)
    int f32_mode = BK_F32_EXACT;  // fp32 rows: widened onto the fp64 MFMA, or the fp32 MFMA
    int f64_mode = BK_F64_EXACT;  // fp64 rows: the fp64 MFMA, or K1i8 (bk_set_f64_mode)
    // hipGraph replay of bk_multikrum_device (bk_graph_enable): one captured
    // launch sequence per call signature; every workspace reallocation or plan
    // eviction bumps ws_epoch, which retires the graphs that baked the old
    // pointers in
    int graph_on = 0;
    uint64_t ws_epoch = 0;
    struct CachedGraph {
        const void *X;
        int dtype;
        int64_t n, d, ld, f;
        const void *sel, *scores, *mean;
        uint64_t epoch;
        hipGraph_t g;
        hipGraphExec_t exec;
    };
    std::vector<CachedGraph> graphs;
    // RCCL
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    int deterministic = 0;
    // the sharded entry's status agreement (sharded_once): the signature of the
    // last agreed call, and the device word the agreement all-reduces
    int64_t agreed_n = -1, agreed_f = -1;
    int agreed_dtype = -1, agreed_det = -1;
    DevBuf status;
    int test_fail_exchange = 0;  // test knob BK_TEST_FAIL_BEFORE_EXCHANGE (bk_create)
    int test_i8_enomem = 0;      // test knob BK_TEST_I8_ENOMEM: K1i8's workspace "fails" (bk_create)
    int test_fail_piece = 0;     // test knob BK_TEST_FAIL_PIECE=p: the overlapped Gram's piece p-1 fails
    int test_pieces_disagree = 0;  // test knob BK_TEST_PIECES_DISAGREE=1: act as if a peer cut the pieces differently
    // the overlapped exchange's piece layout as agreed at the signature's first
    // call: false when the ranks' layouts differed (every rank then exchanges
    // whole, serially, for that signature)
    bool overlap_agreed = true;
    // split scoring (stage_finish): at n >= split_min_n each rank of a sharded
    // call scores its share of the rows and the ranks all-gather the scores
    // (BK_SPLIT_SCORES_MIN_N; 0 turns it off).  Knobs for a 1-rank
    // communicator (bk_create): BK_TEST_SPLIT_SCORES=R scores in R row chunks,
    // one launch each, as R ranks would (the arithmetic of the split, tested on
    // one GPU); BK_EMU_SPLIT_SCORES=R scores only rank 0's chunk once a mode's
    // first call has scored them all (bench.py --emulate-ranks: one rank's time;
    // TIMING ONLY -- the other shares keep that first call's scores, so the
    // outputs and the margin of later calls are not valid, and new data at the
    // same n is not rescored)
    int64_t split_min_n = 2049;
    int test_split_scores = 0, emu_split_scores = 0;
    int test_split_fail = 0;   // BK_TEST_SPLIT_FAIL=p: under BK_TEST_SPLIT_SCORES, share p - 1 "fails"
    int64_t emu_split_n = -1;  // emulation: the n whose other chunks are scored
    DevBuf sgather;            // the gathered scores: parts x chunk doubles
    DevBuf pcnt;               // the overlapped exchange's per-piece arrival counts
    // bk_comm_set_mode 2: the exchange overlapped with the Gram in this many
    // pieces (BK_OVERLAP_PIECES, default 2; 0: off), all-reduced on cstream
    int overlap = 0;
    hipStream_t cstream = nullptr;
    hipEvent_t ev_piece[8] = {};
    hipEvent_t ev_cdone = nullptr;
    unsigned *sigcnt[8] = {};       // probe A/B only (BK_PIECES_DEVWAIT): signal memory for hipStreamWaitValue32
    // the pieces' completion words, polled by the host: fine-grained pinned
    // host memory, one 64-B line per piece (the Gram's last workgroup of a
    // piece stores 1 there, system scope)
    unsigned *hsig = nullptr;       // host address
    unsigned *hsig_d = nullptr;     // the same words as the device addresses them
    bool sig_pending = false;       // a launched Gram's piece words not all seen yet
    int wait_value_ok = -1;         // hipDeviceAttributeCanUseStreamWaitValue (-1: not asked)
    int64_t exchanges = 0;        // exchanges of the packed Gram (bk_comm_stats)
    double exchanged_bytes = 0;   // bytes each rank put into them
    // bk_collect_*: the incremental collection (bk_collect.hip), which owns its
    // buffers -- none of the workspace above, so batch calls leave it intact
    bk::Collect *collect = nullptr;
    // bk_block_*: the miner's block (bk_block_api.hip), buffers of its own as well
    bk::Block *block = nullptr;
    // its cuts (bk_create: BK_BLOCK_MAPPED_HOST / _PINNED / BK_BLOCK_FIN, bytes,
    // for tools/block_bench.py's measurement of the paths on either side)
    int64_t block_mapped_host = bk::BLOCK_MAPPED_HOST_MAX;
    int64_t block_mapped_pinned = bk::BLOCK_MAPPED_PINNED_MAX;
    int64_t block_fin_max = bk::BLOCK_FIN_MAX;
    // bk_eval*: the evaluation sets (bk_eval.hip), created by the first set
    bk::Eval *eval = nullptr;
    // bk_block_finish_eval: the evaluation queued behind the finish, both
    // sharing one wait -- 1: where that measured ahead (the finish is a D2H
    // copy), 2 (BK_BLOCK_EVAL_SEQ=0): everywhere, 0 (BK_BLOCK_EVAL_SEQ=1):
    // nowhere, the finish and the evaluation one after the other.  The outputs
    // are the same bits either way
    int block_eval_one_wait = 1;
    // bk_shares_*: the share state (bk_shares_api.hip), created by the first call
    bk::Shares *shares = nullptr;
    // k_shares_gen's layout: 0 one thread per (chunk, share), 1 one thread per
    // chunk (BK_SHARES_GEN_PER_CHUNK, for tools/shares_bench.py; the same bits)
    int shares_gen_per_chunk = 0;
    // bk_grad*: the training shard and a step's scratch (bk_grad_api.hip),
    // created by the first bk_grad_set_*
    bk::Grad *grad = nullptr;
    // bk_commit_*: the commitment key and a call's scratch (bk_commit_api.hip),
    // created by the first bk_commit_set_key
    bk::Commit *commit = nullptr;
};

namespace bk {

// Split scoring over the ranks of a sharded call (after the
// exchange every rank holds the whole Gram, and K2 -- n sorts of n distances,
// 0.2 ms at n = 4,096 -- was repeated on every rank): rank r scores rows
// [r ch, r ch + ch), ch = ceil(n / parts), into slice r of a parts x (ch + 1)
// buffer whose last word is the rank's status (0, or NaN when its share
// failed), and ONE in-place RCCL all-gather hands every rank all n scores.
// Each row's score is K2's, bitwise, whichever rank computes it.
// k_split_unpack then copies the scores to the caller's array and hands K3b
// the Gram's trailing record, made NaN if any rank's status is not 0 -- so a
// rank that failed its share marks the call invalid on every rank
// (MARGIN_POISONED), as a shard that fails before the exchange does.  Only on
// the transposed K2 path (n >= 2049), whose contiguous diagonal K3b reads
// instead of the per-row diag K2 writes for its own rows only.
enum { SPLIT_NONE = 0, SPLIT_RCCL = 1, SPLIT_TEST = 2, SPLIT_EMU = 3 };
struct ScoreSplit {
    int mode = SPLIT_NONE;
    int parts = 1, part = 0;
};

// bk_api.hip
int ensure(DevBuf &b, size_t bytes);
int get_event(bk_ctx *c, hipEvent_t *out);
bool timing_on(bk_ctx *c, int kid);
int check_common(bk_ctx *c, const void *X, int dtype, int64_t n, int64_t d, int64_t ld);
size_t esize(int dtype);
bool certified(const bk_ctx *c, int dtype);
// bk_stage.hip
void free_plan(Plan3 &p);
int get_plan3(bk_ctx *c, int64_t n, int64_t d, int bk, Plan3 **out);
int v3_bk(int dtype);
bool f32_mfma_now(const bk_ctx *c, int dtype);
bk_ctx::I8Cached *i8_prepared(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d,
                              int64_t ld);
int prepare_gram(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld);
int poison_upper(bk_ctx *c, double *U, int64_t n);
int stage_gram(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
               double *U, Plan &pl);
int gram_pieces(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int k,
                const Pieces **out);
int prepare_finish(bk_ctx *c, int64_t n, const ScoreSplit &sp, bool own_scores);
int stage_finish(bk_ctx *c, const double *U, const Plan &pl, const void *dX, int dtype,
                 int64_t n, int64_t d, int64_t ld, int64_t f, int64_t *d_sel, double *d_scores,
                 double *d_mean, const ScoreSplit &sp = ScoreSplit());
constexpr size_t HOUT_MPAD = 16;  // doubles kept for the record at the head of c->hout
int ensure_hout(bk_ctx *c, size_t words);
int ensure_small_queue(bk_ctx *c);
// the polls a wait of the next one-launch kernel may spend: the test knob's
// (BK_SMALL_SPIN_MAX=<polls>[,<launches>]) while it has launches left
inline uint64_t next_spin(bk_ctx *c) {
    const uint64_t spin = c->small_spin_left == 0 ? SMALL_SPIN_MAX : c->small_spin_max;
    if (c->small_spin_left > 0) --c->small_spin_left;
    return spin;
}
bool small_ok(const bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld);
int run_small(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int64_t f,
              int64_t *d_sel, double *d_scores, double *d_mean, double *margin_out = nullptr,
              double *scores_out = nullptr, int g0 = 0, int gn = -1, bool sm = true);
int run_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int64_t f,
               int64_t *d_sel, double *d_scores, double *d_mean);
hipError_t wait_stream(bk_ctx *c);
int margin_status(const double *mg);
int read_margin(bk_ctx *c, double (&mg)[MARGIN_WORDS]);
int check_margin_readback(bk_ctx *c);
// bk_batch.hip
int ragged_stage_slot(bk_ctx *c, size_t bytes, int *slot);
int batch_fetch(bk_ctx *c);
void batch_pick_record(bk_ctx *c);
// bk_eval.hip: bk_eval in the pieces bk_block_finish_eval shares.  check_args
// needs no context; check_sets, queue and collect run under the context mutex
// with the device selected.  queue launches on the context stream (dw: the
// model on the device); collect reads the mapped block once the stream is done
void eval_destroy(Eval *e);
int eval_check_args(const int *sets, int nsets, const double *err, const int64_t *wrong);
int eval_check_sets(bk_ctx *c, int64_t d, const int *sets, int nsets);
int eval_queue(bk_ctx *c, const double *dw, const int *sets, int nsets);
void eval_collect(bk_ctx *c, int nsets, double *err, int64_t *wrong, int32_t *near_ties);
// bk_host.hip
int stage_host_pipelined(bk_ctx *c, const void *X, int64_t ld, int dtype, const double *noise,
                         int64_t k, int64_t noise_ld, int64_t n, int64_t d, char *dX,
                         int64_t dld, double *U, Plan &pl);

// Error paths of the host entries: queued H2D copies may still read the
// caller's buffers, so both streams are drained unless the entry disarms this.
struct HostDrain {
    bk_ctx *c;
    bool armed = true;
    ~HostDrain() {
        if (!armed) return;
        if (c->copy) (void)hipStreamSynchronize(c->copy);
        (void)hipStreamSynchronize(c->stream);
    }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Bracket one launch with events when timing is on (timing_on).
template <typename F>
int timed(bk_ctx *c, int kid, F &&launch) {
    hipEvent_t a = nullptr, b = nullptr;
    const bool on = timing_on(c, kid);
    if (on) {
        CHK(get_event(c, &a));
        CHK(get_event(c, &b));
        HIPCHK(hipEventRecord(a, c->stream));
    }
    hipError_t e = launch();
    if (e != hipSuccess)
        return fail(BK_EHIP, "%s launch: %s", kKernelNames[kid], hipGetErrorString(e));
    if (on) {
        HIPCHK(hipEventRecord(b, c->stream));
        c->pending.push_back({kid, a, b});
    }
    return BK_OK;
}

// BK_F32_CERTIFIED: run on the fp32 MFMA; if the selection margin does not
// clear the fp32 error bound, run again on the exact path (fp32 widened onto
// the fp64 MFMA), whose outputs replace the first run's.  Synchronous (the
// decision needs the margin on the host).  In the sharded entry every rank
// holds the same summed Gram, hence the same margin and the same decision, so
// the re-run's exchange is joined by all ranks.
template <typename F>
int run_certified(bk_ctx *c, F &&run) {
    CHK(run());
    double mg[MARGIN_WORDS];
    CHK(read_margin(c, mg));
    // only a near tie of a call whose Gram ran on the fp32 MFMA (u_G > 2^-53)
    // is re-run: an exact first pass (k_small, n <= 128) would repeat itself
    if (mg[2] == 0.0 || !(mg[8] > 0x1p-53)) return BK_OK;
    // (BK_EMU_SPLIT_SCORES, timing only: the exact re-run's Gram is another
    // one, so its first call scores every share again, and so does the next
    // approximate call -- ADVICE r5)
    c->emu_split_n = -1;
    c->force_exact = 1;
    const int st = run();
    c->force_exact = 0;
    c->emu_split_n = -1;
    if (st == BK_OK) ++c->certified_reruns;
    return st;
}

}  // namespace bk
