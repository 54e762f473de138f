// bk_collect_arrive_noised.hip -- the last arrival of a NOISED incremental
// collection, noised and finished in ONE launch (include/bk.h
// bk_collect_add_noised_finish).
//
// bk_collect_add_noised followed by bk_collect_finish is four launches behind
// two host calls (k_collect_noise, k_border, k_border_reduce, k_collect_small).
// k_collect_arrive_noised is k_collect_arrive's queue (bk_collect_arrive.hip)
// with the noise of the ONE new row in front -- N, B, S, M:
//
//   N items  (one per chunk  k_collect_noise's arithmetic on the columns of
//             of row j)      chunk s of the new row j: a pair of columns per
//                            lane, out[c] = delta[c] + ((0 + v_0[c]) + .. +
//                            v_{k-1}[c]) / k, j ascending from 0.0, then the
//                            divide, then the add, no contraction; 16-B loads
//                            where a vector's base is 16-B aligned, two 8-B
//                            loads where a BK_DEVICE row is not; the last
//                            column of an odd d alone, 8 bytes; the pad columns
//                            [d, ld) never written.  The k vectors' pointers
//                            travel in the kernel arguments (no table upload)
//   B items  arrive_border (bk_arrive_items.h), after the N items' flag
//   S items  arrive_row + small_rank_sum, after the B items' flag
//   M items  the staging after the N items' flag, small_mean after the S items'
//
// The first N items go to workgroups by blockIdx (they wait for nothing), the
// rest of the queue is dequeued in order: an item only waits for items before
// it, and the grid is at most num_cu workgroups, all resident -- no deadlock.
// Hand-offs are k_small's write-through form and nothing else (wg_arrive /
// wg_raise / wg_wait_flag): the N phase counts on the lines of k_small's former
// reduce phase (C_R, R_GRP, F_R: idle in every collection finish), the B phase
// on the G phase's as in k_collect_arrive.  Queue words, time-out, error word
// and the last workgroup's reset are k_small's.
//
// What is new against k_collect_arrive, and how each hazard is closed:
//  1. ROW j IS WRITTEN INSIDE THE LAUNCH (until now a copy queued before the
//     launch put it there).  Every element of it is an sc1 store, each storing
//     wave drains vmcnt(0), a workgroup barrier, one lane's arrive; the last N
//     item in raises F_R.  Every read of row j comes after a wait on F_R and is
//     an sc1 load; resident rows stay plain loads.  The reads:
//       - the B items' rj: sc1 16-B loads (arrive_border<double, true>);
//       - the B item's ri on the diagonal (i = j): rj's registers, no load;
//       - the M items' staging, which k_collect_arrive runs BEFORE its wait on
//         F_S with plain loads of the store: here it follows a wait on F_R and
//         takes slot j's element by an sc1 load (arrive_mean_stage).
//     No other item reads the store (the S items read the Gram).
//  2. IN PLACE.  For host rows the delta sits in the store row the N item
//     overwrites: each element is read and written by the same thread, and no
//     other thread reads it before F_R.
//  3. THE QUEUE STAYS DEADLOCK-FREE: see above; a wait that gives up sets the
//     error word, and the last workgroup out marks the outputs invalid
//     (small_last_out).  On that BK_EHIP, or a HIP error after the copies were
//     queued, the host does not count the row (bk_collect_add_finish's rule).
#include "bk_arrive_items.h"

namespace bk {

namespace {

struct CollectArriveNoisedArgs {
    CollectArriveArgs a;
    const double *delta;  // row j itself (host rows: uploaded there) or the caller's device row
    const double *vec[COLLECT_ARRIVE_NOISE_MAX_K];  // the k noise vectors, column 0 first
    int k;
};

// columns c, c + 1 of a row whose base is p - c (c even: p is 16-B aligned iff
// the base is -- wave-uniform)
__device__ __forceinline__ d2v noise_pair(const double *p) {
    if (((uintptr_t)p & 15) == 0) return __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p));
    d2v v;
    v.x = __builtin_nontemporal_load(p);
    v.y = __builtin_nontemporal_load(p + 1);
    return v;
}

// N item s: the columns of chunk s of row j, k_collect_noise's arithmetic and
// load shapes; the stores are sc1 (the row is handed to the B and M items)
__device__ __forceinline__ void arrive_noise(const CollectArriveNoisedArgs &na, const SmallArgs &b,
                                             int s, int tid) {
    constexpr int KC = COLLECT_BORDER_CHUNK_BYTES / 8;  // columns per chunk
    const int k = na.k;
    const double dk = (double)k;
    const double *delta = na.delta;
    double *out = (double *)const_cast<void *>(b.X) + (int64_t)na.a.j * b.ld;
    const unsigned nbytes = (unsigned)(b.ld * 8);
    for (int p = tid; p < KC / 2; p += SMALL_NT) {
        const int64_t c = (int64_t)s * KC + 2 * p;
        if (c + 1 < b.d) {
            d2v sum = {0.0, 0.0};
            int j = 0;
            for (; j + 8 <= k; j += 8) {
                d2v v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = noise_pair(na.vec[j + q] + c);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    sum.x += v[q].x;
                    sum.y += v[q].y;
                }
            }
            for (; j < k; ++j) {
                const d2v v = noise_pair(na.vec[j] + c);
                sum.x += v.x;
                sum.y += v.y;
            }
            const d2v x = noise_pair(delta + c);
            d2v o;
            o.x = x.x + sum.x / dk;
            o.y = x.y + sum.y / dk;
            st1_16(out, nbytes, (unsigned)(c * 8), o);
        } else if (c < b.d) {  // the last column of an odd d
            double sum = 0.0;
            for (int j = 0; j < k; ++j) sum += __builtin_nontemporal_load(na.vec[j] + c);
            st1(out + c, __builtin_nontemporal_load(delta + c) + sum / dk);
        }
    }
}

// small_mean_stage on the row store with slot jnew written inside the launch:
// its element is an sc1 load, every resident row's a plain load (the caller has
// waited for the N items' flag)
template <int NB>
__device__ __forceinline__ void arrive_mean_stage(const SmallArgs &a, int c, int tid, double *cols,
                                                  const uint16_t *ord, int jnew) {
    if (!a.mean) return;
    const int cl = tid & 63, r0 = tid >> 6;
    const int64_t col = (int64_t)c * 64 + cl;
    const double *X = (const double *)a.X + (col < a.d ? col : a.d - 1);
    constexpr int RU = 16 * NB / SMALL_NW;
    double v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        const int r = r0 + SMALL_NW * u;
        const int slot = (int)ord[r < a.n ? r : a.n - 1];
        const double *p = X + (int64_t)slot * a.ld;
        v[u] = slot == jnew ? ld1(p) : *p;
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) cols[(r0 + SMALL_NW * u) * 64 + cl] = v[u];
}

}  // namespace

// Items 0..S-1 are the N items (the first min(S, grid) of them held by
// blockIdx), then the nbi B items, the n S items and the M items:
// k_collect_arrive's loop with one more phase in front.  T: the store's
// element type, double (noise is fp64 only)
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_arrive_noised(CollectArriveNoisedArgs na) {
    static_assert(sizeof(T) == 8, "noise is fp64 only");
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
    static_assert(ARRIVE_MAX_S <= 32 * (S_GRP - R_GRP), "the N items' arrival groups");
    const CollectArriveArgs &aa = na.a;
    const SmallArgs &a = aa.c.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nN = aa.S, nbi = aa.nbi;
    const int total = nN + nbi + a.n + a.C;
    unsigned *ctr = a.ctr;
    if (tid < 128) ord[tid] = aa.c.order[tid];  // (the item loop's first barrier follows)
    const int S0 = nN < (int)gridDim.x ? nN : (int)gridDim.x;
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
        if (it < nN) {
            arrive_noise(na, b, it, ot);
            if (wg_arrive(ctr, C_R, R_GRP, it, nN, &s_old)) wg_raise(ctr, F_R);
        } else if (it < nN + nbi) {
            const int bi = it - nN;
            wg_wait_flag(ctr, F_R, a.spin_max);
            arrive_border<T, true>(aa, b, bi, ot, cols);
            if (wg_arrive(ctr, C_G, G_GRP, bi, nbi, &s_old)) wg_raise(ctr, F_G);
        } else if (it < nN + nbi + a.n) {
            const int i = it - nN - nbi;
            wg_wait_flag(ctr, F_G, a.spin_max);
            // the S item's Gram row lives in the (idle) M columns
            arrive_row<NB>(b, aa.c.G, aa.j, ord, i, ot, cols);
            small_rank_sum<NB>(b, i, ot, kbuf, sbuf, rk, cols, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, i, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            const int c = it - nN - nbi - a.n;
            wg_wait_flag(ctr, F_R, a.spin_max);
            arrive_mean_stage<NB>(b, c, ot, cols, ord, aa.j);
            wg_wait_flag(ctr, F_S, a.spin_max);
            small_mean<NB>(b, c, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk, cols, nullptr);
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
}

hipError_t launch_collect_arrive_noised(const void *store, int64_t ld, int j, const double *delta,
                                        const double *const *vecs, int k, int n, int64_t d, int f,
                                        double *G, const int64_t *order, double *scores,
                                        double *diag, int64_t *sel, double *mean, double *margin,
                                        double *scores_out, unsigned *ctr, int num_cu,
                                        hipStream_t st, uint64_t spin_max, int check_lines) {
    if (k < 1 || k > COLLECT_ARRIVE_NOISE_MAX_K || !delta || !vecs) return hipErrorInvalidValue;
    CollectArriveNoisedArgs na = {};
    if (!collect_arrive_fill(na.a, store, 0, ld, j, n, d, f, G, order, scores, diag, sel, mean,
                             margin, scores_out, ctr, spin_max, check_lines))
        return hipErrorInvalidValue;
    na.delta = delta;
    na.k = k;
    for (int q = 0; q < k; ++q) na.vec[q] = vecs[q];
    const int total = na.a.S + na.a.nbi + n + na.a.c.s.C;
    const int grid = total < num_cu ? total : num_cu;
    BK_NB_LAUNCH((n + 15) / 16, k_collect_arrive_noised, grid, st, na, double)
    return hipGetLastError();
}

}  // namespace bk
