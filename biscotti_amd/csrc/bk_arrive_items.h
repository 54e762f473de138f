// bk_arrive_items.h -- what the two fused last-arrival kernels share:
// k_collect_arrive (bk_collect_arrive.hip) and k_collect_arrive_noised
// (bk_collect_arrive_noised.hip).  The argument block, the B item (the border
// of the one new row, the bits of k_border + k_border_reduce) and the S item's
// Gram row with the new run handed off inside the launch.  The kernels' item
// loops are NOT here: each kernel keeps its own, written out.
// k_collect_arrive_wide (bk_collect_arrive_wide.hip) takes the vector types and
// arrive_row from here.  Private to those files; in an unnamed namespace, as bk_collect_arrive.hip
// held them: the kernels keep internal linkage, and k_collect_arrive the code
// and registers it had.
#pragma once
#include "bk_small_items.h"

namespace bk {

namespace {

typedef float af4 __attribute__((ext_vector_type(4)));
template <typename T>
struct ArriveVec;
template <>
struct ArriveVec<double> {
    typedef d2v type;
    static constexpr int N = 2;
};
template <>
struct ArriveVec<float> {
    typedef af4 type;
    static constexpr int N = 4;
};

constexpr int ARRIVE_VPL = COLLECT_BORDER_CHUNK_BYTES / 16 / 64;  // 16-B loads per lane per chunk
constexpr int ARRIVE_MAX_S = 32;  // chunks of a row at small_ok's d <= 32,768 (fp64)
static_assert((int64_t)32768 * 8 <= (int64_t)ARRIVE_MAX_S * COLLECT_BORDER_CHUNK_BYTES,
              "one wave's lanes hold a row's chunk partials");

struct CollectArriveArgs {
    CollectSmallArgs c;
    double *Gw;  // the Gram again, for the B items' stores
    int j;       // the arriving slot
    int S;       // chunks of a row
    int R;       // resident rows per B item: R S <= max(SMALL_NW, S) (chunk, row) units
    int nbi;     // B items: ceil((j + 1) / R)
};

// B item it: rows i = it R .. of the border.  Unit u = (row u / S, chunk u % S)
// goes to wave u % SMALL_NW; the chunk partials meet in part[] (LDS), then wave
// r sums row r's in k_border_reduce's order and lane 0 stores the element.
// NEW1 (k_collect_arrive_noised, fp64): row j was written inside this launch by
// other workgroups, so every load of it is an sc1 load, and the diagonal's ri
// (i = j) is rj's registers, not a second, plain load of the same bytes
template <typename T, bool NEW1 = false>
__device__ __forceinline__ void arrive_border(const CollectArriveArgs &aa, const SmallArgs &b,
                                              int it, int tid, double *part) {
    typedef typename ArriveVec<T>::type V;
    constexpr int N = ArriveVec<T>::N;
    constexpr int KC = COLLECT_BORDER_CHUNK_BYTES / 16 * N;  // columns per chunk
    static_assert(!NEW1 || sizeof(T) == 8, "the noised arrival is fp64 only");
    const int wave = tid >> 6, lane = tid & 63;
    const int S = aa.S, j = aa.j;
    const int r0 = it * aa.R;
    const int nr = j + 1 - r0 < aa.R ? j + 1 - r0 : aa.R;
    const T *store = (const T *)b.X;
    for (int u = wave; u < nr * S; u += SMALL_NW) {
        const int i = r0 + u / S, s = u % S;
        const int64_t c0 = (int64_t)s * KC;
        const T *ri = store + (int64_t)i * b.ld + c0;
        const T *rj = store + (int64_t)j * b.ld + c0;
        V x[ARRIVE_VPL], y[ARRIVE_VPL];
        if constexpr (NEW1) {
            // (the chunk's 16-B vectors below ld: rows are whole vectors long)
            const double *base = (const double *)b.X + (int64_t)j * b.ld;
            const unsigned nbytes = (unsigned)(b.ld * 8);
#pragma unroll
            for (int t = 0; t < ARRIVE_VPL; ++t) {
                const int q = t * 64 + lane;
                const bool in = c0 + (int64_t)q * N < b.d;
                V z = {};
                const V v = ld1_16(base, nbytes, (unsigned)((c0 + (int64_t)(in ? q : 0) * N) * 8));
                y[t] = in ? v : z;
            }
            if (i == j) {  // (wave-uniform)
#pragma unroll
                for (int t = 0; t < ARRIVE_VPL; ++t) x[t] = y[t];
            } else {
#pragma unroll
                for (int t = 0; t < ARRIVE_VPL; ++t) {
                    const int q = t * 64 + lane;
                    const bool in = c0 + (int64_t)q * N < b.d;
                    V z = {};
                    x[t] = in ? reinterpret_cast<const V *>(ri)[q] : z;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < ARRIVE_VPL; ++t) {
                const int q = t * 64 + lane;
                const bool in = c0 + (int64_t)q * N < b.d;  // whole 16-B vectors: the pad columns are 0
                V z = {};
                x[t] = in ? reinterpret_cast<const V *>(ri)[q] : z;
                y[t] = in ? reinterpret_cast<const V *>(rj)[q] : z;
            }
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
        if (lane == 0) part[u] = v;
    }
    __syncthreads();
    if (wave < nr) {
        double v = 0.0;
        for (int s = lane; s < S; s += 64) v += part[wave * S + s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) st1(aa.Gw + (int64_t)j * (j + 1) / 2 + r0 + wave, v);
    }
}

// collect_row with the new run handed off inside the launch: an element of run
// j (its higher slot is j) is an sc1 load, every other one a plain load
template <int NB>
__device__ __forceinline__ void arrive_row(const SmallArgs &a, const double *G, int jnew,
                                           const uint16_t *ord, int i, int tid, double *gv) {
    const int j = tid & 127;
    if (tid < 256 && j < a.n) {
        const int64_t oj = ord[j], oi = tid < 128 ? (int64_t)ord[i] : oj;
        const int64_t hi = oi > oj ? oi : oj, lo = oi > oj ? oj : oi;
        const double *p = G + hi * (hi + 1) / 2 + lo;
        gv[(tid < 128 ? 0 : 16 * NB) + j] = hi == jnew ? ld1(p) : *p;
    }
    __syncthreads();
}

// launch_collect_arrive's argument fill, shared with launch_collect_arrive_noised;
// false when the shape is outside the fused range
static inline bool collect_arrive_fill(CollectArriveArgs &aa, const void *store, int dtype,
                                       int64_t ld, int j, int n, int64_t d, int f, double *G,
                                       const int64_t *order, double *scores, double *diag,
                                       int64_t *sel, double *mean, double *margin,
                                       double *scores_out, unsigned *ctr, uint64_t spin_max,
                                       int check_lines) {
    if (n < 1 || n > 128 || j < 0 || j > 127) return false;
    const int64_t S = (d * (dtype == 0 ? 8 : 4) + COLLECT_BORDER_CHUNK_BYTES - 1) /
                      COLLECT_BORDER_CHUNK_BYTES;
    if (S < 1 || S > ARRIVE_MAX_S) return false;
    if (!collect_small_fill(aa.c, (int)((d + 63) / 64), store, ld, n, d, f, G, order, scores, diag,
                            sel, mean, margin, scores_out, ctr, spin_max, check_lines))
        return false;
    aa.Gw = G;
    aa.j = j;
    aa.S = (int)S;
    aa.R = S >= SMALL_NW ? 1 : SMALL_NW / (int)S;
    aa.nbi = (j + aa.R) / aa.R;
    return true;
}

}  // namespace

}  // namespace bk
