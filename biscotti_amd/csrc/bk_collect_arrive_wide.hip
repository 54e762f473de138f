// bk_collect_arrive_wide.hip -- the last arrival of a WIDE row and its finish
// in ONE launch (include/bk.h bk_set_collect_wide_arrive, bk_collect_add_finish).
//
// k_collect_arrive (bk_collect_arrive.hip) folds the border of the one new row
// into k_collect_small's launch for d <= 32,768, where a border element's chunk
// partials (at most 32) meet in one workgroup's LDS.  A wide row has 33..1,024
// chunks of COLLECT_BORDER_CHUNK_BYTES, so here the border is spread over the
// grid and its partials meet through memory -- the collection's P buffer, at
// k_border's index -- in k_border_reduce's fixed order, inside the same
// persistent queue as k_collect_wide's score and mean items:
//
//   B items  (chunk s, a     k_border's arithmetic for C = 1: the new row's
//             block of rpb   chunk is staged once per item (LDS, then each
//             resident       lane's 8 vectors in registers); a wave streams one
//             rows)          row i <= j of the block with 8 non-temporal 16-B
//                            loads per lane, one fp64 fma per element in load
//                            order (fp32 widened first), the vector's elements
//                            added in order, the lanes by the xor butterfly
//                            32..1 -> P[s (j + 1) + i], an sc1 store
//   R items  (8 elements     after the B items' flag: k_border_reduce's
//             i <= j, one    arithmetic -- lane l adds the partials of chunks
//             wave each)     l, l + 64, .. (sc1 loads) onto 0.0, the same
//                            butterfly -> G[j (j + 1) / 2 + i], an sc1 store
//   S items  (one per row)   k_collect_wide's, after the R items' flag; the
//                            elements of run j are sc1 loads (arrive_row)
//   M items  (2,048 columns) k_collect_wide's, after the S items' flag
//
// wide_arrive_queue / wide_arrive_decode (bk_internal.h) number the items; the
// first min(nB, grid) B items go to workgroups by blockIdx (they wait for
// nothing), the rest of the queue is dequeued in order: an item only waits for
// items before it, so no co-residency is assumed.  Hand-offs are k_small's
// write-through form and nothing else (sc1 stores, each storing wave's
// vmcnt(0), a workgroup barrier, one lane's agent-scope arrive), on lines a
// collection finish leaves idle: the B items on the G phase's (C_G, G_GRP,
// F_G), the R items on the former reduce phase's (C_R, R_GRP, F_R).  Older
// runs of G were written by earlier launches and the new row by a copy queued
// before this one: plain loads.  Queue words, time-out, error word and the last
// workgroup's reset are k_small's.
#include "bk_arrive_items.h"
#include "bk_wide_items.h"

namespace bk {

namespace {

static_assert(WIDE_ARRIVE_NW == SMALL_NW, "one row of a B item, one element of an R item per wave");
static_assert(WIDE_ARRIVE_MAX_B <= 32 * (R_GRP - G_GRP), "the B items arrive on G_GRP's lines");
static_assert((128 + WIDE_ARRIVE_NW - 1) / WIDE_ARRIVE_NW <= 32 * (S_GRP - R_GRP),
              "the R items arrive on R_GRP's lines");

struct CollectArriveWideArgs {
    CollectSmallArgs c;  // k_collect_wide's arguments (s.C = the wide M items)
    double *Gw;          // the Gram again, for the R items' stores
    double *P;           // chunk partials: P[s (j + 1) + i]
    int j;               // the arriving slot
    WideArriveQueue q;
};

// B item (chunk s, row block rb): lv holds the new row's chunk
template <typename T>
__device__ __forceinline__ void wide_arrive_border(const CollectArriveWideArgs &wa,
                                                   const SmallArgs &b, int s, int rb, int tid,
                                                   typename ArriveVec<T>::type *lv) {
    typedef typename ArriveVec<T>::type V;
    constexpr int N = ArriveVec<T>::N;
    constexpr int VPC = COLLECT_BORDER_CHUNK_BYTES / 16;  // 16-B vectors per row chunk
    const int wave = tid >> 6, lane = tid & 63;
    const int j = wa.j;
    const T *store = (const T *)b.X;
    const int64_t c0 = (int64_t)s * (VPC * N);
    for (int v = tid; v < VPC; v += SMALL_NT) {
        const int64_t col = c0 + (int64_t)v * N;  // whole 16-B vectors: the pad columns are 0
        V x = {};
        if (col < b.d) x = *reinterpret_cast<const V *>(store + (int64_t)j * b.ld + col);
        lv[v] = x;
    }
    __syncthreads();
    V y[ARRIVE_VPL];
#pragma unroll
    for (int t = 0; t < ARRIVE_VPL; ++t) y[t] = lv[t * 64 + lane];
    const int r0 = rb * wa.q.rpb;
    const int r1 = r0 + wa.q.rpb < j + 1 ? r0 + wa.q.rpb : j + 1;
    for (int i = r0 + wave; i < r1; i += SMALL_NW) {
        const T *row = store + (int64_t)i * b.ld + c0;
        V x[ARRIVE_VPL];
#pragma unroll
        for (int t = 0; t < ARRIVE_VPL; ++t) {
            const int q = t * 64 + lane;
            V z = {};
            x[t] = c0 + (int64_t)q * N < b.d
                       ? __builtin_nontemporal_load(reinterpret_cast<const V *>(row) + q)
                       : z;
        }
        double acc[N];
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = 0.0;
#pragma unroll
        for (int t = 0; t < ARRIVE_VPL; ++t)
#pragma unroll
            for (int e = 0; e < N; ++e)
                acc[e] = __builtin_fma((double)x[t][e], (double)y[t][e], acc[e]);
        double v = acc[0];
#pragma unroll
        for (int e = 1; e < N; ++e) v += acc[e];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) st1(wa.P + (int64_t)s * (j + 1) + i, v);
    }
}

// R item: elements i0 .. i0 + cnt of run j, one wave each
__device__ __forceinline__ void wide_arrive_reduce(const CollectArriveWideArgs &wa, int i0, int cnt,
                                                   int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    const int j = wa.j, S = wa.q.S;
    if (wave < cnt) {  // (wave-uniform)
        const int i = i0 + wave;
        double v = 0.0;
        for (int s = lane; s < S; s += 64) v += ld1(wa.P + (int64_t)s * (j + 1) + i);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) st1(wa.Gw + (int64_t)j * (j + 1) / 2 + i, v);
    }
}

}  // namespace

// k_collect_wide's loop with two more phases in front
template <typename T, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_collect_arrive_wide(CollectArriveWideArgs wa) {
    typedef typename ArriveVec<T>::type V;
    __shared__ int s_item;
    __shared__ unsigned s_old;
    __shared__ __attribute__((aligned(16))) V lv[COLLECT_BORDER_CHUNK_BYTES / 16];  // B: the new row's chunk
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
    const SmallArgs &a = wa.c.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nB = wa.q.nB, nR = wa.q.nR;
    const int total = nB + nR + a.n + a.C;
    unsigned *ctr = a.ctr;
    if (tid < 128) ord[tid] = wa.c.order[tid];  // (the item loop's first barrier follows)
    const int S0 = nB < (int)gridDim.x ? nB : (int)gridDim.x;
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ctr, C_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int it = __builtin_amdgcn_readfirstlane(s_item);
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
        int kind, x, y;
        wide_arrive_decode(wa.q, wa.j + 1, it, kind, x, y);
        if (kind == WIDE_ARRIVE_B) {
            wide_arrive_border<T>(wa, b, x, y, ot, lv);
            if (wg_arrive(ctr, C_G, G_GRP, it, nB, &s_old)) wg_raise(ctr, F_G);
        } else if (kind == WIDE_ARRIVE_R) {
            wg_wait_flag(ctr, F_G, a.spin_max);
            wide_arrive_reduce(wa, x, y, ot);
            if (wg_arrive(ctr, C_R, R_GRP, it - nB, nR, &s_old)) wg_raise(ctr, F_R);
        } else if (kind == WIDE_ARRIVE_S) {
            wg_wait_flag(ctr, F_R, a.spin_max);
            arrive_row<NB>(b, wa.c.G, wa.j, ord, x, ot, gv);
            small_rank_sum<NB>(b, x, ot, kbuf, sbuf, rk, gv, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, x, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            wg_wait_flag(ctr, F_S, a.spin_max);
            wide_rank_select<NB>(b, x == 0, ot, wave, ot & 63, kbuf, srow, dgl, bnd, balw, rk);
            if (b.mean) wide_mean<T>(b, x, ot, srow, ord, roff);
        }
    }
    if (last_out) small_last_out(a, ctr, tid);
}

hipError_t launch_collect_arrive_wide(const void *store, int dtype, int64_t ld, int j, int n,
                                      int64_t d, int f, double *G, double *P, const int64_t *order,
                                      double *scores, double *diag, int64_t *sel, double *mean,
                                      double *margin, double *scores_out, unsigned *ctr, int num_cu,
                                      hipStream_t st, uint64_t spin_max, int check_lines) {
    // whole 16-B vectors of 16-B aligned rows: the row store's layout
    const int64_t per16 = dtype == 0 ? 2 : 4;
    if (j < 0 || j > 127 || ld < d || !P || !G || ((uintptr_t)store & 15) != 0 || ld % per16 != 0)
        return hipErrorInvalidValue;
    CollectArriveWideArgs wa = {};
    if (!wide_arrive_queue(wa.q, j + 1, d, dtype, n, mean != nullptr)) return hipErrorInvalidValue;
    if (!collect_small_fill(wa.c, collect_wide_items(d), store, ld, n, d, f, G, order, scores, diag,
                            sel, mean, margin, scores_out, ctr, spin_max, check_lines))
        return hipErrorInvalidValue;
    wa.Gw = G;
    wa.P = P;
    wa.j = j;
    const int total = wa.q.nB + wa.q.nR + wa.q.nS + wa.q.nM;
    if (wa.q.nS != n || wa.q.nM != wa.c.s.C) return hipErrorInvalidValue;
    const int grid = total < num_cu ? total : num_cu;
    if (dtype == 0)
        BK_NB_LAUNCH((n + 15) / 16, k_collect_arrive_wide, grid, st, wa, double)
    else
        BK_NB_LAUNCH((n + 15) / 16, k_collect_arrive_wide, grid, st, wa, float)
    return hipGetLastError();
}

}  // namespace bk
