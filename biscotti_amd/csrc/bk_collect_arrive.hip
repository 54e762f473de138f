// bk_collect_arrive.hip -- the last arrival of an incremental collection and
// its finish in ONE launch (include/bk.h bk_collect_add_finish).
//
// The threshold-th update is appended and Krum runs in the same critical
// section (krum.go:291-314).  bk_collect_add followed by bk_collect_finish is
// one copy and three launches (k_border, k_border_reduce, k_collect_small)
// behind two host calls; k_collect_arrive is k_collect_small's queue
// (bk_small.hip) with the border of the ONE new row in front:
//
//   B items  (R resident   <x_i, x_j> of the new slot j with slots i <= j, the
//             rows each)   bits of k_border + k_border_reduce: per chunk of
//                          COLLECT_BORDER_CHUNK_BYTES one wave, lane l's 8
//                          16-B loads ascending, one fp64 fma per element
//                          (fp32 widened first), the vector's elements added
//                          in order, the lanes by the xor butterfly 32..1;
//                          then lane l adds the chunks l, l + 64, .. from 0.0
//                          and the same butterfly.  small_ok bounds d to
//                          32,768, so a row has at most 32 chunks: their
//                          partials meet in LDS, no P buffer.  -> G[j(j+1)/2+i]
//   S items  (one per row) collect_row + small_rank_sum, after the B items'
//                          flag; the elements of run j are sc1 loads
//   M items  (64 columns)  small_mean_stage + small_mean, after the S items'
//                          flag, unchanged
//
// The first B items go to workgroups by blockIdx (they wait for nothing), the
// rest of the queue is dequeued in order: an item only waits for items before
// it.  Hand-offs are k_small's write-through form and nothing else: every
// element of run j is an sc1 store, each storing wave drains vmcnt(0), a
// workgroup barrier, one lane's agent-scope arrive (wg_arrive on the G phase's
// lines, idle in a collection finish); every load of run j by an S item is an
// sc1 load.  Older runs were written by earlier launches: plain loads.  The new
// row itself reached the store by a copy queued before the launch.  Queue
// words, time-out, error word and the last workgroup's reset are k_small's.
// The B item and the S item's Gram row live in bk_arrive_items.h, shared with
// k_collect_arrive_noised (bk_collect_arrive_noised.hip), which noises the new
// row inside the launch too.
#include "bk_arrive_items.h"

namespace bk {

// Items 0..nbi-1 are the B items (the first min(nbi, grid) of them held by
// blockIdx), then the n S items, then the M items: k_collect_small's loop with
// one more phase in front
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_arrive(CollectArriveArgs aa) {
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
    static_assert(16 * NB * 64 >= ARRIVE_MAX_S && ARRIVE_MAX_S >= SMALL_NW,
                  "the B items keep their chunk partials in the (idle) M columns");
    const SmallArgs &a = aa.c.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nbi = aa.nbi;
    const int total = nbi + a.n + a.C;
    unsigned *ctr = a.ctr;
    if (tid < 128) ord[tid] = aa.c.order[tid];  // (the item loop's first barrier follows)
    const int S0 = nbi < (int)gridDim.x ? nbi : (int)gridDim.x;
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
        if (it < nbi) {
            arrive_border<T>(aa, b, it, ot, cols);
            if (wg_arrive(ctr, C_G, G_GRP, it, nbi, &s_old)) wg_raise(ctr, F_G);
        } else if (it < nbi + a.n) {
            const int i = it - nbi;
            wg_wait_flag(ctr, F_G, a.spin_max);
            // the S item's Gram row lives in the (idle) M columns
            arrive_row<NB>(b, aa.c.G, aa.j, ord, i, ot, cols);
            small_rank_sum<NB>(b, i, ot, kbuf, sbuf, rk, cols, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, i, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            const int c = it - nbi - a.n;
            small_mean_stage<T, NB>(b, c, ot, cols, [&](int r) { return (int)ord[r]; });
            wg_wait_flag(ctr, F_S, a.spin_max);
            small_mean<NB>(b, c, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk, cols, nullptr);
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
}

hipError_t launch_collect_arrive(const void *store, int dtype, int64_t ld, int j, int n, int64_t d,
                                 int f, double *G, const int64_t *order, double *scores,
                                 double *diag, int64_t *sel, double *mean, double *margin,
                                 double *scores_out, unsigned *ctr, int num_cu, hipStream_t st,
                                 uint64_t spin_max, int check_lines) {
    CollectArriveArgs aa = {};
    if (!collect_arrive_fill(aa, store, dtype, ld, j, n, d, f, G, order, scores, diag, sel, mean,
                             margin, scores_out, ctr, spin_max, check_lines))
        return hipErrorInvalidValue;
    const int total = aa.nbi + n + aa.c.s.C;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH((n + 15) / 16, k_collect_arrive, grid, st, aa, double)
    else
        BK_NB_LAUNCH((n + 15) / 16, k_collect_arrive, grid, st, aa, float)
    return hipGetLastError();
}

}  // namespace bk
