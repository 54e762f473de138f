// bk_small_ragged.hip -- W independent Multi-Krum problems in ONE launch, every
// problem with its own rows, its own n and its own f (bk_multikrum_ragged*,
// bk_batch.hip): k_small_batch's item loop (bk_small_batch.hip) with
// k_collect_small_ragged's descriptor view and segment search
// (bk_collect_ragged.hip), and k_tiny with one workgroup per descriptor.  The
// item bodies and the hand-off code are bk_small_items.h's, shared with
// k_small; a translation unit of its own, so every other kernel compiles
// exactly as it did without it.
#include "bk_small_items.h"

namespace bk {

// k_small_ragged<T, VEC, NB>: the G, S and M items of W problems, every problem
// with ceil(n / 16) = NB and all of one d (the bucket rule: the item bodies
// choose their shapes from NB, the partials' stride and the G and M item counts
// follow from NB and d, and the single call launches k_small<T, VEC, NB> with
// the same P and C, so problem p's outputs are bitwise what k_small gives on it
// alone).
//
// Queue order, k_small_batch's lag-one pipeline over the problems:
//
//   G_0 | G_1 S_0 M_0 | G_2 S_1 M_1 | ... | G_{W-1} S_{W-2} M_{W-2} | S_{W-1} M_{W-1}
//
// with NGI G items and C M items per problem and n_p S items for problem p; the
// W + 2 segment starts come from the host (ragged_batch_seg_build) and an item
// finds its segment by a wave-uniform binary search over them
// (ragged_batch_queue_decode).  The invariant is k_small's: S_p waits for F_G
// of problem p alone and M_p for F_S of problem p alone, both raised by items
// EARLIER in the queue, with k_small's poll (spin_max bounded); the leading run
// of G items (G_0, and G_1 when there is one, capped by the grid) is held by
// blockIdx and waits for nothing.  No co-residency is assumed.  The
// descriptors and the segment starts are written by the host before the launch
// and by nothing in it.  The last workgroup out resets the launch's lines and
// every problem's; a give-up in any wait marks EVERY problem of the launch
// invalid at the caller's positions (sel = -1, the record's timeout code).
struct RaggedBatchArgs {
    SmallArgs s;  // what the problems share (X = row 0 of the packed matrix, ld, d, P, C, gn = P,
                  // g0 = 0, sm = 1, spin_max) and the bases of the caller-order outputs; part:
                  // slot 0's partials; ctr: problem 0's lines
    const RaggedBatchDesc *desc;  // W problems, in queue order
    const int32_t *seg;           // W + 2 segment starts
    int W, total, lead;           // problems; items (seg[W + 1]); the leading G items (G_0 and G_1)
    int64_t ps;                   // doubles from one slot's partials to the next one's
    unsigned *qh;                 // the launch's own lines: C_HEAD and C_ERR
};

// Problem p's view of the arguments, from its descriptor (p wave-uniform: every
// lane loads the same words, uni() moves them to scalar registers).  n, f and
// the slot are read once per dequeued item, ahead of the item's barrier; the
// offsets are read by the item kinds that use them (ragged_view_*), so a G item
// holds none of the output offsets in registers.
// What every item needs: n, f and the problem's queue lines and partials
__device__ __forceinline__ void ragged_view_common(SmallArgs &b, const RaggedBatchDesc &r, int64_t ps) {
    const int slot = uni(r.slot);
    b.n = uni(r.n);
    b.f = uni(r.f);
    b.nS = b.n;
    b.T = (b.n + 63) / 64;
    b.part += (int64_t)slot * ps;
    b.ctr += (int64_t)slot * SMALL_CTR_WORDS;
}
// G and M items: the problem's rows
template <typename T>
__device__ __forceinline__ void ragged_view_rows(SmallArgs &b, const RaggedBatchDesc &r) {
    b.X = (const T *)b.X + uni(r.row) * b.ld;
}
// S and M items: the problem's scores and diag
__device__ __forceinline__ void ragged_view_scores(SmallArgs &b, const RaggedBatchDesc &r) {
    const int64_t sc = uni(r.sc);
    b.scores += sc;
    b.diag += sc;
}
// M items: the problem's sel, mean and record, at the caller's positions
__device__ __forceinline__ void ragged_view_outputs(SmallArgs &b, const RaggedBatchDesc &r) {
    const int idx = uni(r.idx);
    if (b.mean) b.mean += (int64_t)idx * b.d;
    b.margin += (int64_t)idx * MARGIN_WORDS;
    b.sel += uni(r.so);
}

__device__ __forceinline__ void small_ragged_last_out(const RaggedBatchArgs &ra, int tid) {
    __shared__ unsigned s_err;
    const SmallArgs &a = ra.s;
    // (W opaque: the loops' predicates are formed here, not ahead of the item
    // loop, where the NB = 8 instantiations had no register left to carry one
    // and spilled it)
    int W = ra.W;
    asm volatile("" : "+s"(W));
    if (tid == 0) s_err = ctr_load(cline(ra.qh, C_ERR));
    __syncthreads();
    if (s_err) {  // a wait gave up: every problem of the launch is invalid (small_last_out)
        for (int p = tid; p < W; p += SMALL_NT) {
            const int64_t at = (int64_t)ra.desc[p].idx * MARGIN_WORDS;
            a.margin[at] = __builtin_nan("");
            a.margin[at + 2] = MARGIN_HANDOFF_TIMEOUT;
        }
        for (int p = 0; p < W; ++p) {
            const int m = ra.desc[p].m;
            int64_t *sel = a.sel + ra.desc[p].so;
            for (int i = tid; i < m; i += SMALL_NT) sel[i] = -1;
        }
    }
    __syncthreads();
    // only word 0 of each line is ever written; slot q's lines follow slot q - 1's
    for (int w = tid; w < W * C_LINES; w += SMALL_NT)
        __hip_atomic_store(a.ctr + (int64_t)(w / C_LINES) * SMALL_CTR_WORDS + 32 * (w % C_LINES), 0u,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < C_LINES)
        __hip_atomic_store(ra.qh + 32 * tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T, bool VEC, int NB>
__global__ __launch_bounds__(SMALL_NT) void k_small_ragged(RaggedBatchArgs ra) {
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
    const SmallArgs &a = ra.s;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int NGI = SMALL_SPLIT * a.gn;  // G items per problem
    const int total = ra.total;
    // the leading run of G items (G_0, and G_1 when there is one) goes to
    // workgroups by blockIdx: they wait for nothing
    const int S0 = ra.lead < (int)gridDim.x ? ra.lead : (int)gridDim.x;
    bool last_out = false;
    for (bool first = true;; first = false) {
        if (first && (int)blockIdx.x < S0) {
            if (tid == 0) s_item = (int)blockIdx.x;
        } else if (tid == 0) {
            s_item = S0 + (int)__hip_atomic_fetch_add(cline(ra.qh, C_HEAD), 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const int git = __builtin_amdgcn_readfirstlane(s_item);
        // global item -> (problem p, k_small's item number it of that problem)
        int p = 0, it = 0;
        if (git < total) ragged_batch_queue_decode(ra.seg, ra.W, NGI, git, p, it);
        p = uni(p);
        it = uni(it);
        // the item's view of the arguments and of the thread index, opaque to
        // the optimizer (k_small: nothing hoisted out of the item loop)
        const RaggedBatchDesc &r = ra.desc[p];
        SmallArgs b = a;
        ragged_view_common(b, r, ra.ps);
        asm volatile("" : "+s"(b.n), "+s"(b.f), "+s"(b.P), "+s"(b.C), "+s"(b.d), "+s"(b.ld));
        int ot = tid;
        asm volatile("" : "+v"(ot));
        const int olane = ot & 63;
        unsigned *ctr = b.ctr;
        const int n = b.n;
        __syncthreads();
        if (git >= total) {
            // every workgroup ends on exactly one failed dequeue; the last of
            // them (its add returned total - S0 + grid - 1) is the last one out
            last_out = git == total + (int)gridDim.x - 1;
            break;
        }
        if (it < NGI) {
            ragged_view_rows<T>(b, r);
            small_gram<T, VEC, NB>(b, it, wave, olane, tile, &wbuf[wave][0]);
            if (wg_arrive(ctr, C_G, G_GRP, it, NGI, &s_old)) wg_raise(ctr, F_G);
        } else if (it < NGI + n) {
            ragged_view_scores(b, r);
            wg_wait_flag_on(ctr, F_G, a.spin_max, [&] { return cline(ra.qh, C_ERR); });
            d2v *gv2 = reinterpret_cast<d2v *>(tile);
            double *gv = reinterpret_cast<double *>(tile) + 4 * 16 * NB;
            small_scores<NB>(b, it - NGI, ot, kbuf, sbuf, rk, gv, gv2, red, nullptr);
            if (wg_arrive(ctr, C_S, S_GRP, it - NGI, n, &s_old)) wg_raise(ctr, F_S);
        } else {
            ragged_view_rows<T>(b, r);
            ragged_view_scores(b, r);
            ragged_view_outputs(b, r);
            double *cols = reinterpret_cast<double *>(tile);
            small_mean_stage<T, NB>(b, it - NGI - n, ot, cols, [](int r) { return r; });
            wg_wait_flag_on(ctr, F_S, a.spin_max, [&] { return cline(ra.qh, C_ERR); });
            small_mean<NB>(b, it - NGI - n, ot, wave, olane, kbuf, srow, dgl, bnd, balw, rk, cols,
                           nullptr);
        }
    }
    if (last_out) small_ragged_last_out(ra, tid);
}

// k_tiny_ragged: workgroup b is k_tiny on descriptor b (bk_multikrum_ragged*,
// every n <= 16 and d <= 128): no hand-off between workgroups at all, and
// k_tiny's body, so the same bits per problem
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_tiny_ragged(RaggedBatchArgs ra) {
    const RaggedBatchDesc &r = ra.desc[blockIdx.x];
    SmallArgs b = ra.s;
    b.n = uni(r.n);  // (neither partials nor lines here)
    b.f = uni(r.f);
    ragged_view_rows<T>(b, r);
    ragged_view_scores(b, r);
    ragged_view_outputs(b, r);
    tiny_body<T, VEC>(b);
}

// what both launchers fill: the shared arguments and the caller-order bases
static void small_ragged_fill(RaggedBatchArgs &ra, const void *X, int64_t ld, int W, int64_t d,
                              const SmallPlan &p, const RaggedBatchDesc *desc, double *scores,
                              double *diag, int64_t *sel, double *mean, double *margin,
                              uint64_t spin_max) {
    SmallArgs &a = ra.s;
    a.X = X;
    a.ld = ld;
    a.d = d;
    a.kc = p.kc;
    a.P = p.P;
    a.Q = p.Q;
    a.C = mean ? p.C : 1;  // item 0 writes sel and the margin even without a mean
    a.nblk = p.nblk;
    a.g0 = 0;
    a.gn = p.P;
    a.sm = 1;
    a.scores = scores;
    a.diag = diag;
    a.mean = mean;
    a.margin = margin;
    a.sel = sel;
    a.spin_max = spin_max;
    ra.desc = desc;
    ra.W = W;
}

hipError_t launch_small_ragged(const void *X, int dtype, int64_t ld, int W, int NB, int64_t d,
                               const SmallPlan &p, const RaggedBatchDesc *desc, const int32_t *seg,
                               int total, double *part, int64_t part_stride, double *scores,
                               double *diag, int64_t *sel, double *mean, double *margin,
                               unsigned *lines, int num_cu, hipStream_t st, uint64_t spin_max) {
    if (W < 1 || W > SMALL_BATCH_MAX_W || NB < 1 || NB > 8 || NB != p.nb16 || d < 1 || total < 2 ||
        !X || !desc || !seg || !part || !scores || !diag || !sel || !margin || !lines)
        return hipErrorInvalidValue;
    RaggedBatchArgs ra = {};
    small_ragged_fill(ra, X, ld, W, d, p, desc, scores, diag, sel, mean, margin, spin_max);
    ra.s.part = part;
    ra.s.ctr = lines + SMALL_CTR_WORDS;
    ra.seg = seg;
    ra.total = total;  // <= 1,024 x (1,024 + 128 + 512)
    ra.lead = (W > 1 ? 2 : 1) * SMALL_SPLIT_ITEMS * p.P;
    ra.ps = part_stride;
    ra.qh = lines;
    const int grid = total < num_cu ? total : num_cu;
    // 16-B (fp64) / 8-B (fp32) loads as the single call decides them: with an
    // even ld every problem's first row is aligned as row 0 is
    const bool vec = (ld % 2) == 0 && ((uintptr_t)X % (dtype == 0 ? 16 : 8)) == 0;
    if (dtype == 0 && vec)
        BK_NB_LAUNCH(NB, k_small_ragged, grid, st, ra, double, true)
    else if (dtype == 0)
        BK_NB_LAUNCH(NB, k_small_ragged, grid, st, ra, double, false)
    else if (vec)
        BK_NB_LAUNCH(NB, k_small_ragged, grid, st, ra, float, true)
    else
        BK_NB_LAUNCH(NB, k_small_ragged, grid, st, ra, float, false)
    return hipGetLastError();
}

hipError_t launch_tiny_ragged(const void *X, int dtype, int64_t ld, int W, int64_t d,
                              const RaggedBatchDesc *desc, double *scores, double *diag,
                              int64_t *sel, double *mean, double *margin, hipStream_t st) {
    if (W < 1 || d < 1 || d > SMALL_KC || !X || !desc || !scores || !diag || !sel || !margin)
        return hipErrorInvalidValue;
    RaggedBatchArgs ra = {};
    small_ragged_fill(ra, X, ld, W, d, small_plan(16, d, 0), desc, scores, diag, sel, mean, margin,
                      SMALL_SPIN_MAX);
    const bool vec = (ld % 2) == 0 && ((uintptr_t)X % (dtype == 0 ? 16 : 8)) == 0;
    if (dtype == 0 && vec)
        hipLaunchKernelGGL((k_tiny_ragged<double, true>), dim3(W), dim3(256), 0, st, ra);
    else if (dtype == 0)
        hipLaunchKernelGGL((k_tiny_ragged<double, false>), dim3(W), dim3(256), 0, st, ra);
    else if (vec)
        hipLaunchKernelGGL((k_tiny_ragged<float, true>), dim3(W), dim3(256), 0, st, ra);
    else
        hipLaunchKernelGGL((k_tiny_ragged<float, false>), dim3(W), dim3(256), 0, st, ra);
    return hipGetLastError();
}

}  // namespace bk
