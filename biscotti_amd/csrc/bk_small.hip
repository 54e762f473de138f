// bk_small.hip -- the whole Multi-Krum of a SMALL batch in ONE launch.
//
// Biscotti's verifiers run n <= 100 (config B, mnist: 100 x 7,850; config A,
// creditcard: n <= 10, d = 25; usenix-eval runs n = 28..70).  There the six
// dependent launches of the general path (K1, K1b, K2, K3, K3b, K4) ARE the
// cost: each takes 4-9 us however little it computes (rocprof of config B:
// 58 us per step, profiles/r02).  k_small does the same work in one
// persistent launch whose workgroups pull ITEMS from a queue (one returning
// atomic per item) in dependency order:
//
//   G items  (4 per 128    split-K Gram partial of 128 columns: a quarter of
//             columns)     the upper 16x16 blocks of the (n <= 128) Gram
//                          each, fp64 MFMA
//   S items  (one per row) the row's Gram entries and the diagonal summed
//                          over the P partials in a fixed order (no separate
//                          reduce phase), distances, sort by counting, sum of
//                          ranks 1..k in K2's exact shape
//   M items  (64 columns)  stage the item's columns of every row in LDS while
//                          the scores are computed; then rank the n scores
//                          (each item itself: no serial selection step),
//                          compact the selection, mean of the selected rows
//                          ascending from LDS (K4's order); item 0 writes sel
//                          and the margin
//
// The first G items go to workgroups 0.. by blockIdx, the rest are dequeued
// in order.  An item only waits (a relaxed sc1 poll of a counter) for items
// before it: dequeued ones run on running workgroups, and the statically held
// G items wait for nothing, so their workgroups finish once dispatched.  No
// co-residency is assumed, only that every workgroup of the grid (<= one per
// CU) is eventually dispatched (MI355X_MICROARCH.md, "Workgroup dispatch").  Hand-offs are the guide's write-through form ("Valid forms",
// table row 1): EVERY store of handed-off bytes is an sc1 store (agent-scope
// relaxed atomic store), every storing wave drains vmcnt(0), a workgroup
// barrier, then one lane's agent-scope atomic add; EVERY load of them is an
// sc1 load.  No release / acquire fences: a buffer_wbl2 writes back the XCD's
// dirty L2 (~6.5 us with fresh data), which cost the first version 85 us.
// The last workgroup to exit resets the counters for the next launch.  A wait
// gives up after ~1 s and raises an error word instead of hanging the GPU.
// Results are deterministic: every sum has a fixed order.
//
// k_collect_small (below k_small) is the same queue with the S and M items
// only, for the finish of an incremental collection whose Gram already exists.
// k_small_batch (bk_small_batch.hip) is the same queue over W independent
// problems of one shape (bk_multikrum_batch*): per-problem queue lines and partials, one shared item
// head and error word, the problems' phases software-pipelined; k_tiny_batch is
// k_tiny with one workgroup per problem.  k_collect_small_batch
// (bk_collect_batch.hip) is k_collect_small's queue over W orders of one
// collection (bk_collect_finish_batch).
#include "bk_small_items.h"

namespace bk {

template <typename T, bool VEC, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_small(SmallArgs a) {
    __shared__ int s_item;
    __shared__ unsigned s_old;
    __shared__ __attribute__((aligned(16))) char tile[16 * NB * SMALL_GR * 16];  // G: rows x KC columns
    __shared__ uint64_t kbuf[128];                                      // S / selection keys
    __shared__ __attribute__((aligned(16))) double sbuf[128];          // S: the sorted row
    __shared__ int rk[(SMALL_NT / 128 - 1) * 128];                      // partial ranks
    __shared__ double red[4];                                           // S waves
    __shared__ double bnd[2];
    __shared__ double dgl[128];
    __shared__ int srow[128];
    __shared__ uint64_t balw[2];
    __shared__ double wbuf[SMALL_NW][16 * 17];  // G: each wave's block on its way out
    static_assert(16 * NB * SMALL_GR * 16 >= 6 * 16 * NB * 8, "S items keep their sums in the tile");
    const int tid = threadIdx.x, wave = tid >> 6;
    const int NGI = SMALL_SPLIT * a.gn;  // G items: SPLIT per chunk of this launch
    const int total = NGI + (a.sm ? a.n + a.C : 0);
    unsigned *ctr = a.ctr;
    // the first S0 items (G items) go to workgroups by blockIdx, the rest in
    // queue order (one returning atomic each): 256 dequeues on one counter
    // take ~3 us, which delayed the last G item's start by that much
    const int S0 = NGI < (int)gridDim.x ? NGI : (int)gridDim.x;
    bool last_out = false;
    // debug trace: per workgroup {entry, exit} after the item records
    if (a.trace && tid == 0) a.trace[8 * total + 2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ctr, C_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int it = s_item;
        // the item's view of the arguments, opaque to the optimizer: without
        // this, every predicate and constant the items derive from n, f, P, d
        // (row masks, chunk masks, the margin's gamma divisions) was hoisted
        // out of the item loop into a ~2,300-instruction prologue, spilled to
        // VGPR lanes and run cold from the instruction cache: 4.4 us before
        // the first item started
        SmallArgs b = a;
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.P), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;  // the thread index, opaque likewise (per-thread LDS / row offsets)
        asm volatile("" : "+v"(ot));
        const int olane = ot & 63;
        __syncthreads();
        if (it >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = it == total + (int)gridDim.x - 1;
            break;
        }
        long long t0 = 0, m0 = 0;
        if (a.trace && tid == 0) {
            t0 = (long long)__builtin_amdgcn_s_memrealtime();
            m0 = (long long)__builtin_amdgcn_s_memtime();
        }
        if (it < NGI) {
            small_gram<T, VEC, NB>(b, it, wave, olane, tile, &wbuf[wave][0]);
            // (a G-only launch: the kernel boundary is the hand-off)
            if (a.sm && wg_arrive(ctr, C_G, G_GRP, it, NGI, &s_old)) wg_raise(ctr, F_G);
        } else if (it < NGI + a.n) {
            if (NGI > 0) wg_wait_flag(ctr, F_G, a.spin_max);
            if (a.trace && tid == 0) a.trace[8 * it + 1] = (long long)__builtin_amdgcn_s_memrealtime();
            // the S item's chain sums and Gram row live in the (idle) G tile
            d2v *gv2 = reinterpret_cast<d2v *>(tile);
            double *gv = reinterpret_cast<double *>(tile) + 4 * 16 * NB;
            small_scores<NB>(b, it - NGI, ot, kbuf, sbuf, rk, gv, gv2, red,
                         a.trace ? a.trace + 8 * it : nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, it - NGI, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            // while the scores are computed: this item's 64 columns of every
            // row into LDS, so after the scores only LDS work is left
            double *cols = reinterpret_cast<double *>(tile);
            small_mean_stage<T, NB>(b, it - NGI - a.n, ot, cols, [](int r) { return r; });
            wg_wait_flag(ctr, F_S, a.spin_max);
            if (a.trace && tid == 0) a.trace[8 * it + 1] = (long long)__builtin_amdgcn_s_memrealtime();
            small_mean<NB>(b, it - NGI - a.n, ot, wave, olane, kbuf, srow, dgl, bnd, balw, rk, cols,
                       a.trace ? a.trace + 8 * it : nullptr);
        }
        if (a.trace && tid == 0) {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            a.trace[8 * it] = t0;
            a.trace[8 * it + 2] = (long long)__builtin_amdgcn_s_memrealtime();
            a.trace[8 * it + 3] = (long long)hw | ((long long)blockIdx.x << 32);
            a.trace[8 * it + 4] = m0;
            a.trace[8 * it + 5] = (long long)__builtin_amdgcn_s_memtime();
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
    if (a.trace && tid == 0) a.trace[8 * total + 2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();
}

// k_collect_small: the finish of an incremental collection (bk_collect.hip)
// for n <= 128 in ONE launch. The Gram exists already (by arrival slot, lower
// packed: G[h (h + 1) / 2 + l], l <= h, written by earlier launches on the
// stream, so plain loads see it), hence no G items: k_small's S and M items,
// with the caller's row r read at arrival slot order[r] -- the S items' Gram
// row from G, the M items' staged rows from the row store (s.X, s.ld).  The
// order travels in the kernel arguments (slots < BK_MAX_N fit 16 bits), so
// nothing is uploaded before the launch; entries past n are 0.
// (CollectSmallArgs and collect_row, the S item's first half, are
// bk_small_items.h's: shared with the other collection finishes.)
//
// Items 0..n-1 are the S items (the first min(n, grid) of them held by
// blockIdx: they wait for nothing), items n.. the M items (always dequeued;
// they wait for F_S, raised by S items, all numbered before them).  Queue
// words, hand-off form, timeout and reset are k_small's; the two kernels share
// the context's queue lines and stream order keeps their launches apart.
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_small(CollectSmallArgs ca) {
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
            // the S item's Gram row lives in the (idle) M columns
            collect_row<NB>(b, ca.G, ord, it, ot, cols);
            small_rank_sum<NB>(b, it, ot, kbuf, sbuf, rk, cols, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, it, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            small_mean_stage<T, NB>(b, it - a.n, ot, cols, [&](int r) { return (int)ord[r]; });
            wg_wait_flag(ctr, F_S, a.spin_max);
            small_mean<NB>(b, it - a.n, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk, cols,
                           nullptr);
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_tiny(SmallArgs a) {
    tiny_body<T, VEC>(a);
}

bool tiny_ok(int n, int64_t d) {
    static const bool on = [] {
        const char *e = getenv("BK_TINY");  // 0: k_small for every n <= 128 (A/B)
        return !(e && atoi(e) == 0);
    }();
    return on && n <= 16 && d <= SMALL_KC;
}

SmallPlan small_plan(int n, int64_t d, int num_cu) {
    SmallPlan p;
    p.nb16 = (n + 15) / 16;
    p.nblk = p.nb16 * (p.nb16 + 1) / 2;
    (void)num_cu;
    const int64_t kc = SMALL_KC;
    p.kc = (int)kc;
    p.P = (int)((d + kc - 1) / kc);
    p.ng = SMALL_SPLIT * p.P;
    p.Q = 0;   // no reduce items: every S item sums its own row of the partials
    p.nS = n;  // one S item per row
    p.C = (int)((d + 63) / 64);  // M items: 64 columns each
    return p;
}

hipError_t launch_small(const void *X, int dtype, int64_t ld, int n, int64_t d, int f,
                        const SmallPlan &p, double *part, double *U, double *scores, double *diag,
                        int64_t *sel, double *mean, double *margin, unsigned *ctr, int num_cu,
                        hipStream_t st, long long *trace, uint64_t spin_max, int check_lines,
                        double *scores_out, int g0, int gn, bool sm) {
    SmallArgs a;
    a.g0 = g0;
    a.gn = gn < 0 ? p.P : gn;
    a.sm = sm ? 1 : 0;
    a.scores_out = scores_out;
    a.trace = trace;
    a.spin_max = spin_max;
    a.check_lines = check_lines;
    a.X = X;
    a.ld = ld;
    a.d = d;
    a.n = n;
    a.f = f;
    a.kc = p.kc;
    a.P = p.P;
    a.Q = p.Q;
    a.nS = p.nS;
    a.C = mean ? p.C : 1;  // item 0 writes sel and the margin even without a mean
    a.nblk = p.nblk;
    a.T = (n + 63) / 64;
    a.part = part;
    a.U = U;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.sel = sel;
    a.ctr = ctr;
    const int total = SMALL_SPLIT * a.gn + (a.sm ? a.n + a.C : 0);
    const int grid = total < num_cu ? total : num_cu;
    const bool vec = (ld % 2) == 0 && ((uintptr_t)X % (dtype == 0 ? 16 : 8)) == 0;
    if (tiny_ok(n, d) && !trace && g0 == 0 && a.gn == p.P && sm) {  // one workgroup (k_tiny)
        if (scores_out) a.scores = scores_out;  // k_tiny never reads its scores back
        if (dtype == 0 && vec)
            hipLaunchKernelGGL((k_tiny<double, true>), dim3(1), dim3(256), 0, st, a);
        else if (dtype == 0)
            hipLaunchKernelGGL((k_tiny<double, false>), dim3(1), dim3(256), 0, st, a);
        else if (vec)
            hipLaunchKernelGGL((k_tiny<float, true>), dim3(1), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((k_tiny<float, false>), dim3(1), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    if (dtype == 0 && vec)
        BK_NB_LAUNCH(p.nb16, k_small, grid, st, a, double, true)
    else if (dtype == 0)
        BK_NB_LAUNCH(p.nb16, k_small, grid, st, a, double, false)
    else if (vec)
        BK_NB_LAUNCH(p.nb16, k_small, grid, st, a, float, true)
    else
        BK_NB_LAUNCH(p.nb16, k_small, grid, st, a, float, false)
    return hipGetLastError();
}

hipError_t launch_collect_small(const void *store, int dtype, int64_t ld, int n, int64_t d, int f,
                                const double *G, const int64_t *order, double *scores,
                                double *diag, int64_t *sel, double *mean, double *margin,
                                double *scores_out, unsigned *ctr, int num_cu, hipStream_t st,
                                uint64_t spin_max, int check_lines) {
    if (n < 1 || n > 128) return hipErrorInvalidValue;
    CollectSmallArgs ca = {};
    if (!collect_small_fill(ca, (int)((d + 63) / 64), store, ld, n, d, f, G, order, scores, diag, sel,
                            mean, margin, scores_out, ctr, spin_max, check_lines))
        return hipErrorInvalidValue;
    const int total = n + ca.s.C;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH((n + 15) / 16, k_collect_small, grid, st, ca, double)
    else
        BK_NB_LAUNCH((n + 15) / 16, k_collect_small, grid, st, ca, float)
    return hipGetLastError();
}

}  // namespace bk
