// bk_collect_ragged.hip -- W finishes over ONE incremental collection in ONE
// launch, every problem with its own n and f (bk_collect_finish_ragged,
// bk_collect.hip): k_collect_small_batch (bk_collect_batch.hip) with the
// problem's view read from a descriptor, a queue map for unequal problem sizes
// and the outputs at the caller's positions.  The item bodies, the hand-off
// code and the queue lines are bk_small_items.h's, shared with k_collect_small
// and k_collect_small_batch; so are the argument block (CollectRaggedArgs), the
// problem's view (uni, collect_ragged_view), the last workgroup's reset
// (collect_ragged_last_out) and the launcher's argument fill, shared with
// k_collect_wide_ragged (bk_collect_wide.hip).  A translation unit of its own.
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
    collect_ragged_fill(ra, (int)((d + 63) / 64), store, ld, W, d, G, desc, seg, total, lead, orders,
                        scores, diag, sel, mean, margin, lines, spin_max);
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH(NB, k_collect_small_ragged, grid, st, ra, double)
    else
        BK_NB_LAUNCH(NB, k_collect_small_ragged, grid, st, ra, float)
    return hipGetLastError();
}

}  // namespace bk
