// bk_wide_items.h -- the M item of the wide collection finishes
// (k_collect_wide, k_collect_wide_ragged: bk_collect_wide.hip).  The S items,
// the queue words and the hand-off code are bk_small_items.h's, unchanged; an M
// item here owns COLLECT_WIDE_COLS columns and streams the selected rows from
// the row store instead of staging every row's 64 columns in LDS.  Private to
// bk_collect_wide.hip and bk_collect_arrive_wide.hip (k_collect_arrive_wide).
#pragma once
#include "bk_small_items.h"

namespace bk {

// The selection of one problem from its n published scores: small_mean's
// ranking, ballots and margin code (bk_small_items.h) without its staged
// columns.  Every M item ranks the scores itself (n <= 128: one LDS pass, no
// selection hand-off).  On return -- a workgroup barrier has passed -- srow[0 ..
// m) holds the selected rows of the caller ascending and balw the selection
// masks.  The lead item (M item 0) also writes sel, the second copy of the
// scores and the margin record.
template <int NB>
__device__ __forceinline__ void wide_rank_select(const SmallArgs &a, bool lead, int tid, int wave,
                                                 int lane, uint64_t *keys, int *srow, double *dg,
                                                 double *bnd, uint64_t *balw, int *rkm) {
    const int n = a.n, m = n - a.f;
    double si = 0.0;
    if (tid < n) {
        si = ld1(a.scores + tid);
        keys[tid] = dkey(si);
    } else if (tid < 128) {
        keys[tid] = ~0ULL;  // padding: after every real key (NaN included)
    } else if (lead && tid - 128 < n) {
        dg[tid - 128] = ld1(a.diag + tid - 128);
    }
    __syncthreads();
    // rank of row e in the (score, index) total order: the P2 threads of key e
    // count over their parts of the NP = 16 NB (padded) keys
    const int e = tid & 127, h = tid >> 7;
    const uint64_t ki = keys[e];
    constexpr int P2 = SMALL_NT / 128, HK = 16 * NB / P2, U = HK % 8 == 0 ? 8 : 4;
    int cnt = 0;
#pragma unroll
    for (int j0 = 0; j0 < HK; j0 += U) {
        uint64_t o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) o[u] = keys[HK * h + j0 + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = HK * h + j0 + u;
            cnt += (o[u] < ki) || (o[u] == ki && j < e);
        }
    }
    if (h >= 1 && e < n) rkm[(h - 1) * 128 + e] = cnt;
    __syncthreads();
    bool on = false;
    if (h == 0 && e < n) {
#pragma unroll
        for (int q = 1; q < P2; ++q) cnt += rkm[(q - 1) * 128 + e];
        on = cnt < m;
        if (lead && cnt == m - 1) bnd[0] = si;
        if (lead && cnt == m) bnd[1] = si;
        if (lead && a.scores_out) a.scores_out[e] = si;
    }
    // compaction: rows 0..63 in wave 0, 64..127 in wave 1
    const uint64_t bal = __ballot(on);
    if (wave < 2 && lane == 0) balw[wave] = bal;
    __syncthreads();
    if (on) {
        const int pos = (wave ? __popcll(balw[0]) : 0) + __popcll(bal & ((1ull << lane) - 1));
        srow[pos] = tid;
        if (lead && a.sel) a.sel[pos] = (int64_t)tid;
    }
    if (lead && wave == 3) {
        double M = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = lane + 64 * q;
            if (j < n) {
                const double v = dg[j];
                if (v == v && v < __builtin_inf() && v > M) M = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o));
        if (lane == 0) {
            const int64_t k = n - a.f - 2 > 0 ? n - a.f - 2 : 0;
            write_margin(a.margin, bnd[0], bnd[1], M, (double)a.d, k, 0x1p-53);
        }
    }
    __syncthreads();
}

typedef double wd2 __attribute__((ext_vector_type(2)));
typedef float wf4 __attribute__((ext_vector_type(4)));
template <typename T>
struct WideVec;
template <>
struct WideVec<double> {
    typedef wd2 type;
};
template <>
struct WideVec<float> {
    typedef wf4 type;
};

// Wide M item c: columns [c W, c W + W) of the mean, W = COLLECT_WIDE_COLS.
// srow[0 .. m) are the selected rows ascending (wide_rank_select), ord[r] the
// arrival slot of the caller's row r.  Thread t owns VPT 16-B vectors of N
// columns, vector j at column c W + (j NT + t) N, so a wave's loads of one row
// are one contiguous run; row-store rows are 16-B aligned and their pad columns
// [d, ld) exist (and hold 0), so a vector that starts below d is loaded whole.
// DEPTH rows' loads are in flight at once (16 non-temporal 16-B loads per
// thread); a round past m repeats row m - 1 and adds +0.0 instead: acc starts at
// +0.0 and a round-to-nearest sum is -0.0 only if both addends are, so acc is
// never -0.0 and acc + 0.0 == acc bit for bit (small_mean's argument).  One fp64
// accumulator per column, the selected rows added strictly in ascending order
// (fp32 widened first), then K4's own scaling, / m: K4's sum bit for bit for m
// <= 128 (mean_segments(m) == 1), whatever W is.
template <typename T>
__device__ __forceinline__ void wide_mean(const SmallArgs &a, int c, int tid, const int *srow,
                                          const uint16_t *ord, int64_t *roff) {
    typedef typename WideVec<T>::type V;
    constexpr int N = 16 / (int)sizeof(T);
    constexpr int VPT = COLLECT_WIDE_COLS / N / SMALL_NT;
    constexpr int DEPTH = 16 / VPT;
    static_assert(VPT >= 1 && VPT * N * SMALL_NT == COLLECT_WIDE_COLS, "whole vectors per thread");
    static_assert(COLLECT_WIDE_COLS % 64 == 0, "the item width is a multiple of 64");
    const int m = a.n - a.f;
    if (tid < m) roff[tid] = (int64_t)ord[srow[tid]] * a.ld;
    __syncthreads();
    const T *X = (const T *)a.X;
    int64_t col[VPT];
    bool in[VPT];
    double acc[VPT][N];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        col[j] = (int64_t)c * COLLECT_WIDE_COLS + (int64_t)(j * SMALL_NT + tid) * N;
        in[j] = col[j] < a.d;  // (col is a multiple of N and ld = d rounded up to N: the vector fits)
#pragma unroll
        for (int e = 0; e < N; ++e) acc[j][e] = 0.0;
    }
    for (int r0 = 0; r0 < m; r0 += DEPTH) {
        V v[DEPTH][VPT];
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) {
            const int64_t ro = roff[r0 + q < m ? r0 + q : m - 1];
#pragma unroll
            for (int j = 0; j < VPT; ++j)
                v[q][j] = __builtin_nontemporal_load(
                    reinterpret_cast<const V *>(X + ro + (in[j] ? col[j] : 0)));
        }
#pragma unroll
        for (int q = 0; q < DEPTH; ++q) {
            const bool on = r0 + q < m;
#pragma unroll
            for (int j = 0; j < VPT; ++j)
#pragma unroll
                for (int e = 0; e < N; ++e) acc[j][e] += on ? (double)v[q][j][e] : 0.0;
        }
    }
    const double dm = (double)m;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
#pragma unroll
        for (int e = 0; e < N; ++e)
            if (col[j] + e < a.d) a.mean[col[j] + e] = acc[j][e] / dm;
}

}  // namespace bk
