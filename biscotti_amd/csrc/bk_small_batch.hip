// bk_small_batch.hip -- W independent Multi-Krum problems of one shape in ONE
// launch (bk_multikrum_batch*, bk_batch.hip): k_small's queue (bk_small.hip)
// with one more index in front of it, and k_tiny with one workgroup per
// problem.  The item bodies and the hand-off code are bk_small_items.h's, shared
// with k_small; a translation unit of its own, so k_small, k_collect_small and
// k_tiny compile exactly as they did without it.
#include "bk_small_items.h"

namespace bk {

// k_small_batch: W independent problems of one shape (n, d, f) in ONE launch
// (bk_multikrum_batch*): k_small's queue with one more index in front.  The G,
// S and M item bodies, the waits, the arrivals and the hand-off form are
// k_small's own functions, called on problem p's view of the arguments -- its
// rows, its slice of the partials, its outputs and ITS OWN queue lines (arrival
// counters and per-XCD phase flags) -- so problem p's outputs are bitwise what
// k_small gives on it alone.  The item head and the error word are the
// launch's (a line block of their own, ba.qh).
//
// Queue order, a lag-one software pipeline over the problems:
//
//   G_0 | G_1 S_0 M_0 | G_2 S_1 M_1 | ... | G_{W-1} S_{W-2} M_{W-2} | S_{W-1} M_{W-1}
//
// so the S items of problem p are dequeued behind the G items of problem
// p + 1: the workgroups that would poll for G_p's tail have Gram work to do
// first.  The invariant is k_small's: S_p waits for G_p and M_p for S_p, all of
// them EARLIER in the queue, with k_small's poll (spin_max bounded); the
// statically held first items (by blockIdx: the leading run of G items, G_0 and
// G_1, capped by the grid) wait for nothing.  No co-residency is assumed.  The
// last workgroup out resets the launch's lines and every problem's; a give-up
// in any wait marks EVERY problem of the launch invalid (sel = -1, the
// record's timeout code).
struct BatchArgs {
    SmallArgs s;       // problem 0's view (gn = P, g0 = 0, sm = 1; ctr: problem 0's lines)
    int W, m;          // problems of this launch; m = n - f
    int64_t xs;        // bytes from one problem's rows to the next one's
    int64_t ps;        // doubles from one problem's partials to the next one's
    unsigned *qh;      // the launch's own lines: C_HEAD and C_ERR
};

// problem p's view of the arguments (p wave-uniform)
__device__ __forceinline__ void batch_view(SmallArgs &b, int p, int64_t xs, int64_t ps, int m) {
    b.X = (const char *)b.X + (int64_t)p * xs;
    b.part += (int64_t)p * ps;
    b.scores += (int64_t)p * b.n;
    b.diag += (int64_t)p * b.n;
    if (b.mean) b.mean += (int64_t)p * b.d;
    b.margin += (int64_t)p * MARGIN_WORDS;
    b.sel += (int64_t)p * m;
    b.ctr += (int64_t)p * SMALL_CTR_WORDS;
}

__device__ __forceinline__ void small_batch_last_out(const BatchArgs &ba, int tid) {
    __shared__ unsigned s_err;
    const SmallArgs &a = ba.s;
    if (tid == 0) s_err = ctr_load(cline(ba.qh, C_ERR));
    __syncthreads();
    if (s_err) {  // a wait gave up: every problem of the launch is invalid (small_last_out)
        for (int p = tid; p < ba.W; p += SMALL_NT) {
            a.margin[(int64_t)p * MARGIN_WORDS] = __builtin_nan("");
            a.margin[(int64_t)p * MARGIN_WORDS + 2] = MARGIN_HANDOFF_TIMEOUT;
        }
        for (int64_t i = tid; i < (int64_t)ba.W * ba.m; i += SMALL_NT) a.sel[i] = -1;
    }
    __syncthreads();
    // only word 0 of each line is ever written
    for (int w = tid; w < ba.W * C_LINES; w += SMALL_NT)
        __hip_atomic_store(a.ctr + (int64_t)(w / C_LINES) * SMALL_CTR_WORDS + 32 * (w % C_LINES), 0u,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < C_LINES)
        __hip_atomic_store(ba.qh + 32 * tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T, bool VEC, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_small_batch(BatchArgs ba) {
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
    const SmallArgs &a = ba.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int NGI = SMALL_SPLIT * a.gn;      // G items per problem
    const int per = NGI + a.n + a.C;         // items per problem
    const int total = ba.W * per;
    // the leading run of G items (G_0, and G_1 when there is one) goes to
    // workgroups by blockIdx: they wait for nothing
    const int lead = ba.W > 1 ? 2 * NGI : NGI;
    const int S0 = lead < (int)gridDim.x ? lead : (int)gridDim.x;
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ba.qh, C_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int git = __builtin_amdgcn_readfirstlane(s_item);
        // global item -> (problem p, k_small's item number it of that problem)
        int p = 0, it = git;
        if (git >= NGI && git < total) {
            const int r = git - NGI, j = r / per, q = r - j * per;
            if (j < ba.W - 1) {
                p = q < NGI ? j + 1 : j;
                it = q;
            } else {
                p = ba.W - 1;
                it = NGI + q;
            }
        }
        // the item's view of the arguments, opaque to the optimizer (k_small)
        SmallArgs b = a;
        batch_view(b, p, ba.xs, ba.ps, ba.m);
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.P), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;
        asm volatile("" : "+v"(ot));
        const int olane = ot & 63;
        unsigned *ctr = b.ctr;
        __syncthreads();
        if (git >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = git == total + (int)gridDim.x - 1;
            break;
        }
        if (it < NGI) {
            small_gram<T, VEC, NB>(b, it, wave, olane, tile, &wbuf[wave][0]);
            if (wg_arrive(ctr, C_G, G_GRP, it, NGI, &s_old)) wg_raise(ctr, F_G);
        } else if (it < NGI + a.n) {
            wg_wait_flag_on(ctr, F_G, a.spin_max, [&] { return cline(ba.qh, C_ERR); });
            d2v *gv2 = reinterpret_cast<d2v *>(tile);
            double *gv = reinterpret_cast<double *>(tile) + 4 * 16 * NB;
            small_scores<NB>(b, it - NGI, ot, kbuf, sbuf, rk, gv, gv2, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, it - NGI, a.n, &s_old)) wg_raise(ctr, F_S);
        } else {
            double *cols = reinterpret_cast<double *>(tile);
            small_mean_stage<T, NB>(b, it - NGI - a.n, ot, cols, [](int r) { return r; });
            wg_wait_flag_on(ctr, F_S, a.spin_max, [&] { return cline(ba.qh, C_ERR); });
            small_mean<NB>(b, it - NGI - a.n, ot, wave, olane, kbuf, srow, dgl, bnd, balw, rk, cols,
                           nullptr);
        }
    }
    if (last_out) small_batch_last_out(ba, tid);
}

// k_tiny_batch: workgroup b is k_tiny on problem b of a batch of one shape
// (bk_multikrum_batch*, n <= 16 and d <= 128): no hand-off between workgroups
// at all, and k_tiny's body, so the same bits per problem
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_tiny_batch(BatchArgs ba) {
    SmallArgs b = ba.s;
    batch_view(b, (int)blockIdx.x, ba.xs, ba.ps, ba.m);
    tiny_body<T, VEC>(b);
}

hipError_t launch_small_batch(const void *X, int dtype, int64_t ld, int64_t stride, int W, int n,
                              int64_t d, int f, const SmallPlan &p, double *part, int64_t part_stride,
                              double *scores, double *diag, int64_t *sel, double *mean,
                              double *margin, unsigned *lines, int num_cu, hipStream_t st,
                              uint64_t spin_max) {
    if (W < 1 || n < 1 || n > 128 || !sel || !scores || !diag || !margin)
        return hipErrorInvalidValue;
    BatchArgs ba = {};
    SmallArgs &a = ba.s;
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
    a.g0 = 0;
    a.gn = p.P;
    a.sm = 1;
    a.part = part;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.sel = sel;
    a.spin_max = spin_max;
    ba.W = W;
    ba.m = n - f;
    ba.xs = stride * (int64_t)(dtype == 0 ? 8 : 4);
    ba.ps = part_stride;
    // 16-B (fp64) / 8-B (fp32) loads only if every problem's rows allow them
    const bool vec = (ld % 2) == 0 && (W == 1 || (stride % 2) == 0) &&
                     ((uintptr_t)X % (dtype == 0 ? 16 : 8)) == 0;
    if (tiny_ok(n, d)) {  // one workgroup per problem (k_tiny_batch)
        if (dtype == 0 && vec)
            hipLaunchKernelGGL((k_tiny_batch<double, true>), dim3(W), dim3(256), 0, st, ba);
        else if (dtype == 0)
            hipLaunchKernelGGL((k_tiny_batch<double, false>), dim3(W), dim3(256), 0, st, ba);
        else if (vec)
            hipLaunchKernelGGL((k_tiny_batch<float, true>), dim3(W), dim3(256), 0, st, ba);
        else
            hipLaunchKernelGGL((k_tiny_batch<float, false>), dim3(W), dim3(256), 0, st, ba);
        return hipGetLastError();
    }
    if (!part || !lines) return hipErrorInvalidValue;
    ba.qh = lines;
    a.ctr = lines + SMALL_CTR_WORDS;
    const int64_t total = (int64_t)W * (SMALL_SPLIT * a.gn + a.n + a.C);
    if (total > (int64_t)1 << 30) return hipErrorInvalidValue;
    const int grid = total < num_cu ? (int)total : num_cu;
    if (dtype == 0 && vec)
        BK_NB_LAUNCH(p.nb16, k_small_batch, grid, st, ba, double, true)
    else if (dtype == 0)
        BK_NB_LAUNCH(p.nb16, k_small_batch, grid, st, ba, double, false)
    else if (vec)
        BK_NB_LAUNCH(p.nb16, k_small_batch, grid, st, ba, float, true)
    else
        BK_NB_LAUNCH(p.nb16, k_small_batch, grid, st, ba, float, false)
    return hipGetLastError();
}

}  // namespace bk
