// bk_collect_wide.hip -- the one-launch collection finishes for WIDE rows: n <=
// 128 and 32,768 < d <= BK_COLLECT_WIDE_MAX_D, opted into by
// bk_set_collect_wide (bk_collect.hip finish_wide, finish_ragged).
//
// k_collect_small's cap on d belongs to k_small's G items; a collection finish
// has none (the Gram exists), but its M items give every 64 columns an item of
// their own that stages a 16 NB x 64 tile and ranks the scores again -- 4,096
// rankings at d = 262,144.  The kernels here keep k_collect_small's S items
// (collect_row + small_rank_sum), queue words, F_S hand-off, time-out and reset
// exactly, and its numbering rule (S items first, the first min(n, grid) of
// them held by blockIdx, M items always dequeued; an item waits only for items
// numbered before it, so no co-residency is assumed and there is no new kind of
// wait), and replace the M item: item c owns COLLECT_WIDE_COLS columns, ranks
// the scores once and streams the m selected rows from the row store with 16-B
// non-temporal loads into one fp64 accumulator per column (bk_wide_items.h).
//
// k_collect_wide<T, NB>         one finish; the order in the kernel arguments
// k_collect_wide_ragged<T, NB>  W finishes of one NB behind
//                               k_collect_small_ragged's descriptors and queue
//                               map (ragged_seg_build / ragged_queue_decode
//                               with collect_wide_items(d) M items per problem)
//
// A translation unit of its own: every other kernel compiles exactly as it did
// without it.
#include "bk_wide_items.h"

namespace bk {

struct CollectWideArgs {
    SmallArgs s;  // gn = 0, sm = 1; X = the row store; C = the wide M items; part, U, trace unused
    const double *G;
    uint16_t order[128];
};

template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_wide(CollectWideArgs ca) {
    __shared__ int s_item;
    __shared__ unsigned s_old;
    __shared__ __attribute__((aligned(16))) double gv[2 * 16 * NB];  // S: the Gram row, the diagonal
    __shared__ uint64_t kbuf[128];                                    // S / selection keys
    __shared__ __attribute__((aligned(16))) double sbuf[128];        // S: the sorted row
    __shared__ int rk[(SMALL_NT / 128 - 1) * 128];                    // partial ranks
    __shared__ double red[4];                                         // S waves
    __shared__ double bnd[2];
    __shared__ double dgl[128];
    __shared__ int srow[128];
    __shared__ uint64_t balw[2];
    __shared__ uint16_t ord[128];
    __shared__ int64_t roff[128];  // M: the selected rows' offsets in the row store
    const SmallArgs &a = ca.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = a.n + a.C;
    unsigned *ctr = a.ctr;
    if (tid < 128) ord[tid] = ca.order[tid];  // (the item loop's first barrier follows)
    const int S0 = a.n < (int)gridDim.x ? a.n : (int)gridDim.x;
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ctr, C_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int it = s_item;
        // the item's view of the arguments and of the thread index, opaque to
        // the optimizer (k_small: nothing hoisted out of the item loop)
        SmallArgs b = a;
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;
        asm volatile("" : "+v"(ot));
        __syncthreads();
        if (it >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = it == total + (int)gridDim.x - 1;
            break;
        }
        if (it < a.n) {
            collect_row<NB>(b, ca.G, ord, it, ot, gv);
            small_rank_sum<NB>(b, it, ot, kbuf, sbuf, rk, gv, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, it, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            wg_wait_flag(ctr, F_S, a.spin_max);
            wide_rank_select<NB>(b, it == a.n, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk);
            if (b.mean) wide_mean<T>(b, it - a.n, ot, srow, ord, roff);
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
}

struct CollectWideRaggedArgs {
    SmallArgs s;             // what the problems share (X = the row store, ld, d, C, spin_max) and
                             // the bases of the caller-order outputs; ctr: problem 0's lines
    const double *G;         // the collection's Gram by arrival slot, lower packed
    const RaggedDesc *desc;  // W problems, in queue order
    const int32_t *seg;      // W + 2 segment starts
    const uint16_t *orders;  // the packed arrival slots (desc[p].ord)
    int W, total, lead;      // problems; items (seg[W + 1]); the leading S items (S_0 and S_1)
    unsigned *qh;            // the launch's own lines: CBQ_HEAD and CBQ_ERR
};

// a wave-uniform value into scalar registers (the descriptors and the segment
// starts are loaded by vector loads; every lane reads the same word)
__device__ __forceinline__ int wuni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t wuni(int64_t v) {
    return (int64_t)(((uint64_t)(uint32_t)wuni((int)((uint64_t)v >> 32)) << 32) |
                     (uint32_t)wuni((int)v));
}

// problem p's view of the arguments (p wave-uniform), as k_collect_small_ragged
// takes it from its descriptor.  Returns the offset of its order
__device__ __forceinline__ int64_t wide_ragged_view(SmallArgs &b, const RaggedDesc *desc, int p) {
    const RaggedDesc &r = desc[p];
    const int idx = wuni(r.idx);
    const int64_t sc = wuni(r.sc);
    b.n = wuni(r.n);
    b.f = wuni(r.f);
    b.nS = b.n;
    b.scores += sc;
    b.diag += sc;
    if (b.mean) b.mean += (int64_t)idx * b.d;
    b.margin += (int64_t)idx * MARGIN_WORDS;
    b.sel += wuni(r.so);
    b.ctr += (int64_t)p * (CB_LINES * 32);
    return wuni(r.ord);
}

// the last workgroup out: a give-up in any wait marks every problem of the
// launch invalid (sel = -1, the record's time-out code), then the launch's
// lines and every problem's go back to zero
__device__ __forceinline__ void wide_ragged_last_out(const CollectWideRaggedArgs &ra, int tid) {
    __shared__ unsigned s_err;
    const SmallArgs &a = ra.s;
    if (tid == 0) s_err = ctr_load(cline(ra.qh, CBQ_ERR));
    __syncthreads();
    if (s_err) {
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

// Queue order and invariant are k_collect_small_ragged's: the lag-one pipeline
//   S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}
// M_p waits for F_S of problem p alone, raised by S items earlier in the queue;
// S items wait for nothing and the leading run of them is held by blockIdx.
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_wide_ragged(CollectWideRaggedArgs ra) {
    __shared__ int s_item;
    __shared__ unsigned s_old;
    __shared__ __attribute__((aligned(16))) double gv[2 * 16 * NB];  // S: the Gram row, the diagonal
    __shared__ uint64_t kbuf[128];                                    // S / selection keys
    __shared__ __attribute__((aligned(16))) double sbuf[128];        // S: the sorted row
    __shared__ int rk[(SMALL_NT / 128 - 1) * 128];                    // partial ranks
    __shared__ double red[4];                                         // S waves
    __shared__ double bnd[2];
    __shared__ double dgl[128];
    __shared__ int srow[128];
    __shared__ uint64_t balw[2];
    __shared__ uint16_t ord[128];
    __shared__ int64_t roff[128];  // M: the selected rows' offsets in the row store
    const SmallArgs &a = ra.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = ra.total;
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
        // global item -> (problem p, k_collect_wide's item number it of that problem)
        int p = 0, it = 0;
        if (git < total) ragged_queue_decode(ra.seg, ra.W, a.C, git, p, it);
        p = wuni(p);
        it = wuni(it);
        SmallArgs b = a;
        const int64_t oo = wide_ragged_view(b, ra.desc, p);
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
            last_out = git == total + (int)gridDim.x - 1;
            break;
        }
        if (it < n) {
            collect_row<NB>(b, ra.G, ord, it, ot, gv);
            small_rank_sum<NB>(b, it, ot, kbuf, sbuf, rk, gv, red, nullptr);
            if (wg_arrive(ctr, CB_S, CB_GRP, it, n, &s_old)) wg_raise(ctr, CB_F);
        } else {
            wg_wait_flag_on(ctr, CB_F, a.spin_max, [&] { return cline(ra.qh, CBQ_ERR); });
            wide_rank_select<NB>(b, it == n, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk);
            if (b.mean) wide_mean<T>(b, it - n, ot, srow, ord, roff);
        }
    }
    if (last_out) wide_ragged_last_out(ra, tid);
}

#define BK_WIDE_NB_SWITCH(KERNEL, ARGS)                                                          \
    switch (NBv) {                                                                               \
    case 1: hipLaunchKernelGGL((KERNEL<T, 1>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 2: hipLaunchKernelGGL((KERNEL<T, 2>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 3: hipLaunchKernelGGL((KERNEL<T, 3>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 4: hipLaunchKernelGGL((KERNEL<T, 4>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 5: hipLaunchKernelGGL((KERNEL<T, 5>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 6: hipLaunchKernelGGL((KERNEL<T, 6>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    case 7: hipLaunchKernelGGL((KERNEL<T, 7>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break;  \
    default: hipLaunchKernelGGL((KERNEL<T, 8>), dim3(grid), dim3(SMALL_NT), 0, st, ARGS); break; \
    }

template <typename T>
static void launch_collect_wide_t(const CollectWideArgs &a, int NBv, int grid, hipStream_t st) {
    BK_WIDE_NB_SWITCH(k_collect_wide, a)
}

template <typename T>
static void launch_collect_wide_ragged_t(const CollectWideRaggedArgs &a, int NBv, int grid,
                                         hipStream_t st) {
    BK_WIDE_NB_SWITCH(k_collect_wide_ragged, a)
}
#undef BK_WIDE_NB_SWITCH

// the wide M item loads whole 16-B vectors of 16-B aligned rows: the row
// store's layout (bk_collect_begin pads ld and zeroes the pad columns)
static bool wide_rows_ok(const void *store, int dtype, int64_t ld) {
    const int64_t per16 = dtype == 0 ? 2 : 4;
    return ((uintptr_t)store & 15) == 0 && ld % per16 == 0;
}

hipError_t launch_collect_wide(const void *store, int dtype, int64_t ld, int n, int64_t d, int f,
                               const double *G, const int64_t *order, double *scores, double *diag,
                               int64_t *sel, double *mean, double *margin, double *scores_out,
                               unsigned *ctr, int num_cu, hipStream_t st, uint64_t spin_max,
                               int check_lines) {
    if (n < 1 || n > 128 || d < 1 || ld < d || !wide_rows_ok(store, dtype, ld))
        return hipErrorInvalidValue;
    CollectWideArgs ca = {};
    SmallArgs &a = ca.s;
    a.X = store;
    a.ld = ld;
    a.d = d;
    a.n = n;
    a.f = f;
    a.nS = n;
    a.C = mean ? collect_wide_items(d) : 1;  // item 0 writes sel and the margin even without a mean
    a.sm = 1;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.scores_out = scores_out;
    a.sel = sel;
    a.ctr = ctr;
    a.spin_max = spin_max;
    a.check_lines = check_lines;
    ca.G = G;
    for (int i = 0; i < n; ++i) {
        const int64_t o = order ? order[i] : i;
        if (o < 0 || o > 0xFFFF) return hipErrorInvalidValue;
        ca.order[i] = (uint16_t)o;
    }
    const int total = n + a.C;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        launch_collect_wide_t<double>(ca, (n + 15) / 16, grid, st);
    else
        launch_collect_wide_t<float>(ca, (n + 15) / 16, grid, st);
    return hipGetLastError();
}

// (the descriptors are the caller's to validate, as launch_collect_small_ragged's)
hipError_t launch_collect_wide_ragged(const void *store, int dtype, int64_t ld, int W, int NB,
                                      int64_t d, const double *G, const RaggedDesc *desc,
                                      const int32_t *seg, int total, int lead,
                                      const uint16_t *orders, double *scores, double *diag,
                                      int64_t *sel, double *mean, double *margin, unsigned *lines,
                                      int num_cu, hipStream_t st, uint64_t spin_max) {
    if (W < 1 || W > SMALL_BATCH_MAX_W || NB < 1 || NB > 8 || d < 1 || ld < d || total < 2 ||
        lead < 1 || lead >= total || !G || !desc || !seg || !orders || !scores || !diag || !sel ||
        !margin || !lines || !wide_rows_ok(store, dtype, ld))
        return hipErrorInvalidValue;
    CollectWideRaggedArgs ra = {};
    SmallArgs &a = ra.s;
    a.X = store;
    a.ld = ld;
    a.d = d;
    a.C = mean ? collect_wide_items(d) : 1;  // item 0 writes sel and the margin even without a mean
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
    ra.total = total;  // <= 1,024 x (128 + 512)
    ra.lead = lead;
    ra.qh = lines;
    a.ctr = lines + CBQ_LINES * 32;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        launch_collect_wide_ragged_t<double>(ra, NB, grid, st);
    else
        launch_collect_wide_ragged_t<float>(ra, NB, grid, st);
    return hipGetLastError();
}

}  // namespace bk
