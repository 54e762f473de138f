// bk_collect_ragged.hip -- W finishes over ONE incremental collection in ONE
// launch, every problem with its own n and f (bk_collect_finish_ragged,
// bk_collect.hip): k_collect_small_batch (bk_collect_batch.hip) with the
// problem's view read from a descriptor, a queue map for unequal problem sizes
// and the outputs at the caller's positions.  The item bodies, the hand-off
// code and the queue lines are bk_small_items.h's, shared with k_collect_small
// and k_collect_small_batch; a translation unit of its own, so the kernels of
// bk_small.hip, bk_small_batch.hip and bk_collect_batch.hip compile exactly as
// they did without it.
#include "bk_small_items.h"

namespace bk {

// k_collect_small_ragged<T, NB>: the S and M items of W problems over one
// collection, every problem with ceil(n / 16) = NB (the bucket rule: the item
// bodies choose their summation shapes from NB, and the single finish launches
// with the problem's own NB, so only the same instantiation gives its bits).
//
// Queue order, k_collect_small_batch's lag-one pipeline over the problems:
//
//   S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}
//
// with n_p S items and C M items for problem p; the W + 2 segment starts come
// from the host (ragged_seg_build) and an item finds its segment by a
// wave-uniform binary search over them (ragged_queue_decode).  The invariant is
// unchanged: M_p waits for F_S of problem p alone, raised by S items EARLIER
// in the queue, with k_small's poll (spin_max bounded); S items wait for
// nothing, and the leading run of them (S_0, and S_1 when there is one, capped
// by the grid) is held by blockIdx.  No co-residency is assumed.  The
// descriptors, the segment starts and the orders are written by the host
// before the launch and by nothing in it.  The last workgroup out resets the
// launch's lines and every problem's; a give-up in any wait marks EVERY problem
// of the launch invalid (sel = -1, the record's timeout code).
struct CollectRaggedArgs {
    SmallArgs s;             // what the problems share (X = the row store, ld, d, C, spin_max) and
                             // the bases of the caller-order outputs; ctr: problem 0's lines
    const double *G;         // the collection's Gram by arrival slot, lower packed
    const RaggedDesc *desc;  // W problems, in queue order
    const int32_t *seg;      // W + 2 segment starts
    const uint16_t *orders;  // the packed arrival slots (desc[p].ord)
    int W, total, lead;      // problems; items (seg[W + 1]); the leading S items (S_0 and S_1)
    unsigned *qh;            // the launch's own lines: CBQ_HEAD and CBQ_ERR
};

// a wave-uniform value into scalar registers.  The descriptors and the segment
// starts are loaded by vector loads (the kernel stores to global memory, so the
// compiler keeps such loads off the scalar path); every lane reads the same word
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni(int64_t v) {
    return (int64_t)(((uint64_t)(uint32_t)uni((int)((uint64_t)v >> 32)) << 32) |
                     (uint32_t)uni((int)v));
}

// problem p's view of the arguments (p wave-uniform): its descriptor, read once
// per dequeued item.  Returns the offset of its order
__device__ __forceinline__ int64_t collect_ragged_view(SmallArgs &b, const RaggedDesc *desc, int p) {
    const RaggedDesc &r = desc[p];
    const int idx = uni(r.idx);
    const int64_t sc = uni(r.sc);
    b.n = uni(r.n);
    b.f = uni(r.f);
    b.nS = b.n;
    b.scores += sc;
    b.diag += sc;
    if (b.mean) b.mean += (int64_t)idx * b.d;
    b.margin += (int64_t)idx * MARGIN_WORDS;
    b.sel += uni(r.so);
    b.ctr += (int64_t)p * (CB_LINES * 32);
    return uni(r.ord);
}

__device__ __forceinline__ void collect_ragged_last_out(const CollectRaggedArgs &ra, int tid) {
    __shared__ unsigned s_err;
    const SmallArgs &a = ra.s;
    if (tid == 0) s_err = ctr_load(cline(ra.qh, CBQ_ERR));
    __syncthreads();
    if (s_err) {  // a wait gave up: every problem of the launch is invalid (small_last_out)
        for (int p = tid; p < ra.W; p += SMALL_NT) {
            const int64_t at = (int64_t)ra.desc[p].idx * MARGIN_WORDS;
            a.margin[at] = __builtin_nan("");
            a.margin[at + 2] = MARGIN_HANDOFF_TIMEOUT;
        }
        for (int p = 0; p < ra.W; ++p) {
            const int m = ra.desc[p].m;
            int64_t *sel = a.sel + ra.desc[p].so;
            for (int i = tid; i < m; i += SMALL_NT) sel[i] = -1;
        }
    }
    __syncthreads();
    // only word 0 of each line is ever written
    for (int w = tid; w < ra.W * CB_LINES; w += SMALL_NT)
        __hip_atomic_store(a.ctr + 32 * (int64_t)w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < CBQ_LINES)
        __hip_atomic_store(ra.qh + 32 * tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_small_ragged(CollectRaggedArgs ra) {
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
    const SmallArgs &a = ra.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = ra.total;
    // the leading run of S items (S_0, and S_1 when there is one) goes to
    // workgroups by blockIdx: they wait for nothing
    const int S0 = ra.lead < (int)gridDim.x ? ra.lead : (int)gridDim.x;
    int cur = -1;  // the problem whose order is in LDS
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ra.qh, CBQ_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int git = __builtin_amdgcn_readfirstlane(s_item);
        // global item -> (problem p, k_collect_small's item number it of that problem)
        int p = 0, it = 0;
        if (git < total) ragged_queue_decode(ra.seg, ra.W, a.C, git, p, it);
        p = uni(p);
        it = uni(it);
        // the item's view of the arguments and of the thread index, opaque to
        // the optimizer (k_small: nothing hoisted out of the item loop)
        SmallArgs b = a;
        const int64_t oo = collect_ragged_view(b, ra.desc, p);
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;
        asm volatile("" : "+v"(ot));
        unsigned *ctr = b.ctr;
        const int n = b.n;
        // every thread has passed the barrier above, so the previous item's
        // reads of the order are done; the barrier below publishes the new one
        if (git < total && p != cur) {
            if (tid < 128) ord[tid] = tid < n ? ra.orders[oo + tid] : (uint16_t)0;
            cur = p;
        }
        __syncthreads();
        if (git >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = git == total + (int)gridDim.x - 1;
            break;
        }
        if (it < n) {
            // the S item's Gram row lives in the (idle) M columns
            collect_row<NB>(b, ra.G, ord, it, ot, cols);
            small_rank_sum<NB>(b, it, ot, kbuf, sbuf, rk, cols, red, nullptr);
            if (wg_arrive(ctr, CB_S, CB_GRP, it, n, &s_old)) wg_raise(ctr, CB_F);
        } else {
            small_mean_stage<T, NB>(b, it - n, ot, cols, [&](int q) { return (int)ord[q]; });
            wg_wait_flag_on(ctr, CB_F, a.spin_max, [&] { return cline(ra.qh, CBQ_ERR); });
            small_mean<NB>(b, it - n, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk, cols,
                           nullptr);
        }
    }
    if (last_out) collect_ragged_last_out(ra, tid);
}

template <typename T>
static void launch_collect_ragged_t(const CollectRaggedArgs &a, int NBv, int grid, hipStream_t st) {
    switch (NBv) {
    case 1: hipLaunchKernelGGL((k_collect_small_ragged<T, 1>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_collect_small_ragged<T, 2>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_collect_small_ragged<T, 3>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_collect_small_ragged<T, 4>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 5: hipLaunchKernelGGL((k_collect_small_ragged<T, 5>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 6: hipLaunchKernelGGL((k_collect_small_ragged<T, 6>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    case 7: hipLaunchKernelGGL((k_collect_small_ragged<T, 7>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    default: hipLaunchKernelGGL((k_collect_small_ragged<T, 8>), dim3(grid), dim3(SMALL_NT), 0, st, a); break;
    }
}

// (the descriptors are the caller's to validate: every n in 16 NB - 15 .. 16 NB,
// 0 <= f < n, m = n - f, the offsets inside the arrays; seg = ragged_seg_build
// of the n's, total = seg[W + 1], lead = the S items of problems 0 and 1)
hipError_t launch_collect_small_ragged(const void *store, int dtype, int64_t ld, int W, int NB,
                                       int64_t d, const double *G, const RaggedDesc *desc,
                                       const int32_t *seg, int total, int lead,
                                       const uint16_t *orders, double *scores, double *diag,
                                       int64_t *sel, double *mean, double *margin, unsigned *lines,
                                       int num_cu, hipStream_t st, uint64_t spin_max) {
    if (W < 1 || W > SMALL_BATCH_MAX_W || NB < 1 || NB > 8 || d < 1 || total < 2 || lead < 1 ||
        lead >= total || !store || !G || !desc || !seg || !orders || !scores || !diag || !sel ||
        !margin || !lines)
        return hipErrorInvalidValue;
    CollectRaggedArgs ra = {};
    SmallArgs &a = ra.s;
    a.X = store;
    a.ld = ld;
    a.d = d;
    a.C = mean ? (int)((d + 63) / 64) : 1;  // item 0 writes sel and the margin even without a mean
    a.sm = 1;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.sel = sel;
    a.spin_max = spin_max;
    ra.G = G;
    ra.desc = desc;
    ra.seg = seg;
    ra.orders = orders;
    ra.W = W;
    ra.total = total;  // <= 1,024 x 640
    ra.lead = lead;
    ra.qh = lines;
    a.ctr = lines + CBQ_LINES * 32;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        launch_collect_ragged_t<double>(ra, NB, grid, st);
    else
        launch_collect_ragged_t<float>(ra, NB, grid, st);
    return hipGetLastError();
}

}  // namespace bk
