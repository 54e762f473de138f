// bk_collect_batch.hip -- W finishes over ONE incremental collection in ONE
// launch (bk_collect_finish_batch, bk_collect.hip): k_collect_small's queue
// (bk_small.hip) with k_small_batch's extra index in front of it.  Problem p is
// Multi-Krum over the collected rows order_p[0..n) (arrival slots: a subset and
// any permutation); every problem reads the same Gram and the same row store,
// so there is no Gram phase and nothing is uploaded but the W x n slot numbers.
// The item bodies and the hand-off code are bk_small_items.h's, shared with
// k_collect_small; so are the reset of the queue lines (collect_lines_reset,
// shared with the ragged kernels) and the launcher's NB dispatch.  A
// translation unit of its own.
#include "bk_small_items.h"

namespace bk {

// k_collect_small_batch: the S and M items of W problems of one shape (n, f)
// over one collection.  Problem p's view: its own 16-bit order (row p of a
// device array W x n), scores, diag, sel, mean, margin record and queue lines;
// the item head and the error word are the launch's (ba.qh).
//
// Queue order, a lag-one software pipeline over the problems:
//
//   S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}
//
// so the M items of problem p are dequeued behind the S items of problem p + 1:
// the workgroups that would poll for S_p's tail have scores to compute first.
// The invariant is k_small's: M_p waits for F_S of problem p, raised by S
// items EARLIER in the queue, with k_small's poll (spin_max bounded); S items
// wait for nothing, and the leading run of them (S_0, and S_1 when there is
// one, capped by the grid) is held by blockIdx.  No co-residency is assumed.
// A workgroup moves between problems, so it reloads its LDS copy of the order
// whenever the dequeued item's problem changes (a barrier before the first
// use).  The last workgroup out resets the launch's lines and every problem's;
// a give-up in any wait marks EVERY problem of the launch invalid (sel = -1,
// the record's timeout code).
struct CollectBatchArgs {
    SmallArgs s;            // problem 0's view (gn = 0, sm = 1; X = the row store; ctr: problem 0's lines)
    const double *G;        // the collection's Gram by arrival slot, lower packed
    const uint16_t *orders; // W x n arrival slots
    int W, m;               // problems of this launch; m = n - f
    unsigned *qh;           // the launch's own lines: CBQ_HEAD and CBQ_ERR
};

// problem p's view of the arguments (p wave-uniform)
__device__ __forceinline__ void collect_batch_view(SmallArgs &b, int p, int m) {
    b.scores += (int64_t)p * b.n;
    b.diag += (int64_t)p * b.n;
    if (b.mean) b.mean += (int64_t)p * b.d;
    b.margin += (int64_t)p * MARGIN_WORDS;
    b.sel += (int64_t)p * m;
    b.ctr += (int64_t)p * (CB_LINES * 32);
}

__device__ __forceinline__ void collect_batch_last_out(const CollectBatchArgs &ba, int tid) {
    __shared__ unsigned s_err;
    const SmallArgs &a = ba.s;
    if (tid == 0) s_err = ctr_load(cline(ba.qh, CBQ_ERR));
    __syncthreads();
    if (s_err) {  // a wait gave up: every problem of the launch is invalid (small_last_out)
        for (int p = tid; p < ba.W; p += SMALL_NT) {
            a.margin[(int64_t)p * MARGIN_WORDS] = __builtin_nan("");
            a.margin[(int64_t)p * MARGIN_WORDS + 2] = MARGIN_HANDOFF_TIMEOUT;
        }
        for (int64_t i = tid; i < (int64_t)ba.W * ba.m; i += SMALL_NT) a.sel[i] = -1;
    }
    __syncthreads();
    collect_lines_reset(a.ctr, ba.qh, ba.W, tid);
}

template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_small_batch(CollectBatchArgs ba) {
    __shared__ int s_item;
    __shared__ unsigned s_old;
    __shared__ __attribute__((aligned(16))) double cols[16 * NB * 64];  // M: rows x 64 columns
    __shared__ uint64_t kbuf[128];                                      // S / selection keys
    __shared__ __attribute__((aligned(16))) double sbuf[128];          // S: the sorted row
    __shared__ int rk[(SMALL_NT / 128 - 1) * 128];                      // partial ranks
    __shared__ double red[4];                                           // S waves
    __shared__ double bnd[2];
    __shared__ double dgl[128];
    __shared__ int srow[128];
    __shared__ uint64_t balw[2];
    __shared__ uint16_t ord[128];
    const SmallArgs &a = ba.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int per = a.n + a.C;  // items per problem
    const int total = ba.W * per;
    // the leading run of S items (S_0, and S_1 when there is one) goes to
    // workgroups by blockIdx: they wait for nothing
    const int lead = ba.W > 1 ? 2 * a.n : a.n;
    const int S0 = lead < (int)gridDim.x ? lead : (int)gridDim.x;
    int cur = -1;  // the problem whose order is in LDS
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ba.qh, CBQ_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int git = __builtin_amdgcn_readfirstlane(s_item);
        // global item -> (problem p, k_collect_small's item number it of that problem)
        int p = 0, it = git;
        if (git >= a.n && git < total) {
            const int r = git - a.n, j = r / per, q = r - j * per;
            if (j < ba.W - 1) {
                p = q < a.n ? j + 1 : j;
                it = q;
            } else {
                p = ba.W - 1;
                it = a.n + q;
            }
        }
        // the item's view of the arguments and of the thread index, opaque to
        // the optimizer (k_small: nothing hoisted out of the item loop)
        SmallArgs b = a;
        collect_batch_view(b, p, ba.m);
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;
        asm volatile("" : "+v"(ot));
        unsigned *ctr = b.ctr;
        // every thread has passed the barrier above, so the previous item's
        // reads of the order are done; the barrier below publishes the new one
        if (git < total && p != cur) {
            if (tid < 128) ord[tid] = tid < a.n ? ba.orders[(int64_t)p * a.n + tid] : (uint16_t)0;
            cur = p;
        }
        __syncthreads();
        if (git >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = git == total + (int)gridDim.x - 1;
            break;
        }
        if (it < a.n) {
            // the S item's Gram row lives in the (idle) M columns
            collect_row<NB>(b, ba.G, ord, it, ot, cols);
            small_rank_sum<NB>(b, it, ot, kbuf, sbuf, rk, cols, red, nullptr);
            if (wg_arrive(ctr, CB_S, CB_GRP, it, a.n, &s_old)) wg_raise(ctr, CB_F);
        } else {
            small_mean_stage<T, NB>(b, it - a.n, ot, cols, [&](int r) { return (int)ord[r]; });
            wg_wait_flag_on(ctr, CB_F, a.spin_max, [&] { return cline(ba.qh, CBQ_ERR); });
            small_mean<NB>(b, it - a.n, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk, cols,
                           nullptr);
        }
    }
    if (last_out) collect_batch_last_out(ba, tid);
}

hipError_t launch_collect_small_batch(const void *store, int dtype, int64_t ld, int W, int n,
                                      int64_t d, int f, const double *G, const uint16_t *orders,
                                      double *scores, double *diag, int64_t *sel, double *mean,
                                      double *margin, unsigned *lines, int num_cu, hipStream_t st,
                                      uint64_t spin_max) {
    if (W < 1 || W > SMALL_BATCH_MAX_W || n < 1 || n > 128 || f < 0 || f >= n || d < 1 || !store ||
        !G || !orders || !scores || !diag || !sel || !margin || !lines)
        return hipErrorInvalidValue;
    CollectBatchArgs ba = {};
    SmallArgs &a = ba.s;
    a.X = store;
    a.ld = ld;
    a.d = d;
    a.n = n;
    a.f = f;
    a.nS = n;
    a.C = mean ? (int)((d + 63) / 64) : 1;  // item 0 writes sel and the margin even without a mean
    a.sm = 1;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.sel = sel;
    a.spin_max = spin_max;
    ba.G = G;
    ba.orders = orders;
    ba.W = W;
    ba.m = n - f;
    ba.qh = lines;
    a.ctr = lines + CBQ_LINES * 32;
    const int64_t total = (int64_t)W * (n + a.C);  // <= 1,024 x 640
    const int grid = total < num_cu ? (int)total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH((n + 15) / 16, k_collect_small_batch, grid, st, ba, double)
    else
        BK_NB_LAUNCH((n + 15) / 16, k_collect_small_batch, grid, st, ba, float)
    return hipGetLastError();
}

}  // namespace bk
