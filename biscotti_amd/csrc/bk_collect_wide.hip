// bk_collect_wide.hip -- the one-launch collection finishes for WIDE rows: n <=
// 128 and 32,768 < d <= BK_COLLECT_WIDE_MAX_D, opted into by
// bk_set_collect_wide (bk_collect.hip finish_one_launch, finish_ragged).
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
// The argument blocks (CollectSmallArgs, CollectRaggedArgs), the ragged
// problem's view and reset (uni, collect_ragged_view, collect_ragged_invalidate,
// collect_lines_reset) and the launchers' argument fill are k_collect_small's and
// k_collect_small_ragged's own, from bk_small_items.h.  A translation unit of
// its own.
#include "bk_wide_items.h"

namespace bk {

// (s.C = the wide M items)
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_wide(CollectSmallArgs ca) {
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

// collect_ragged_last_out under this kernel's own name (see there: the name
// decides where the kernel's LDS words lie)
__device__ __forceinline__ void wide_ragged_last_out(const CollectRaggedArgs &ra, int tid) {
    __shared__ unsigned s_err;
    if (tid == 0) s_err = ctr_load(cline(ra.qh, CBQ_ERR));
    __syncthreads();
    if (s_err) collect_ragged_invalidate(ra, tid);
    __syncthreads();
    collect_lines_reset(ra.s.ctr, ra.qh, ra.W, tid);
}

// Queue order and invariant are k_collect_small_ragged's: the lag-one pipeline
//   S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}
// M_p waits for F_S of problem p alone, raised by S items earlier in the queue;
// S items wait for nothing and the leading run of them is held by blockIdx.
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_wide_ragged(CollectRaggedArgs ra) {
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
        p = uni(p);
        it = uni(it);
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
    CollectSmallArgs ca = {};
    if (!collect_small_fill(ca, collect_wide_items(d), store, ld, n, d, f, G, order, scores, diag, sel,
                            mean, margin, scores_out, ctr, spin_max, check_lines))
        return hipErrorInvalidValue;
    const int total = n + ca.s.C;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH((n + 15) / 16, k_collect_wide, grid, st, ca, double)
    else
        BK_NB_LAUNCH((n + 15) / 16, k_collect_wide, grid, st, ca, float)
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
    CollectRaggedArgs ra = {};
    collect_ragged_fill(ra, collect_wide_items(d), store, ld, W, d, G, desc, seg, total, lead, orders,
                        scores, diag, sel, mean, margin, lines, spin_max);
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH(NB, k_collect_wide_ragged, grid, st, ra, double)
    else
        BK_NB_LAUNCH(NB, k_collect_wide_ragged, grid, st, ra, float)
    return hipGetLastError();
}

}  // namespace bk
