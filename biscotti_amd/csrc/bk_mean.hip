// bk_mean.hip -- the masked mean of the Multi-Krum engine, CDNA4 (gfx950).
//
// The last step of one Multi-Krum call (DESIGN.md "Kernels"; K1 is in
// bk_gram.hip, K2-K3b in bk_scores.hip):
//   K4  k_mean      masked mean of the selected rows, fp64, ascending order
//                   (logistic_validator.py:51)
//                   (ACCUM: the block aggregation GlobalW += sum, honest.go:361-375)
// and k_synth, the synthetic batch generator (bk_synth.h).
//
// Built with -ffp-contract=off: every add and the divide round exactly as the
// numpy reference evaluates them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_device.h"
#include "bk_internal.h"
#include "bk_synth.h"

namespace bk {

// ---------------------------------------------------------------------------
// K4: mean[c] = (sum over selected rows, ascending) / m      (:51, fp64)
// ---------------------------------------------------------------------------
// ACCUM = false: mean[c] = (sum over r in sel order of X[sel[r]][c]) / m   (K4)
// ACCUM = true:  mean[c] = mean[c] + X[sel[0]][c] + X[sel[1]][c] + ...       (in sel
//                order, sequential: the GlobalW update of honest.go:361-375)
// SEG (a large selection, m >= MEAN_SEG_MIN): block row y sums the selected
// rows [y L, y L + L) into part[y][c] (no divide), k_mean_comb adds the
// segments in order -- a fixed order that depends on m only, so every shard
// and device of one call adds alike
#ifndef BK_MEAN_DEPTH
#define BK_MEAN_DEPTH 8  // rows' loads in flight per thread (same adds in the same order at any depth)
#endif
template <typename T, bool VEC, bool ACCUM = false, bool SEG = false>
__global__ __launch_bounds__(256) void k_mean(const T *__restrict__ X, int64_t ld, int64_t d,
                                              const int64_t *__restrict__ sel, int m,
                                              double *__restrict__ mean) {
    extern __shared__ __attribute__((aligned(16))) int64_t srow[];  // row offsets (elements)
    if constexpr (SEG) {
        const int r0 = (int)blockIdx.y * MEAN_SEG_ROWS;
        sel += r0;
        m = m - r0 < MEAN_SEG_ROWS ? m - r0 : MEAN_SEG_ROWS;
        mean += (int64_t)blockIdx.y * d;
    }
    for (int r = threadIdx.x; r < m; r += 256) srow[r] = sel[r] * ld;
    __syncthreads();
    const double dm = SEG ? 1.0 : (double)m;
    const int64_t npair = (d + 1) >> 1;
    for (int64_t cp = (int64_t)blockIdx.x * 256 + threadIdx.x; cp < npair;
         cp += (int64_t)gridDim.x * 256) {
        const int64_t c = cp * 2;
        if (c + 1 < d) {
            d2v acc = {0.0, 0.0};
            if constexpr (ACCUM) acc = d2v{mean[c], mean[c + 1]};
            int r = 0;
            for (; r + BK_MEAN_DEPTH <= m; r += BK_MEAN_DEPTH) {
                d2v v[BK_MEAN_DEPTH];
#pragma unroll
                for (int q = 0; q < BK_MEAN_DEPTH; ++q) v[q] = ld2s<T, VEC>(X + srow[r + q] + c);
#pragma unroll
                for (int q = 0; q < BK_MEAN_DEPTH; ++q) {
                    acc.x += v[q].x;
                    acc.y += v[q].y;
                }
            }
            for (; r < m; ++r) {
                const d2v v = ld2s<T, VEC>(X + srow[r] + c);
                acc.x += v.x;
                acc.y += v.y;
            }
            if constexpr (ACCUM || SEG) {
                mean[c] = acc.x;
                mean[c + 1] = acc.y;
            } else {
                mean[c] = acc.x / dm;
                mean[c + 1] = acc.y / dm;
            }
        } else {
            double acc = ACCUM ? mean[c] : 0.0;
            for (int r = 0; r < m; ++r) acc += (double)X[srow[r] + c];
            mean[c] = (ACCUM || SEG) ? acc : acc / dm;
        }
    }
}

// fp32 rows with 16-B aligned starts: 4 columns per thread from one 16-B load
// (the f2v form above moves 8 B per load: config E's K4 ran at 3.9 TB/s).  The
// same per-column order of adds as k_mean, so the same bits.
template <bool ACCUM, bool SEG = false>
__global__ __launch_bounds__(256) void k_mean_f4(const float *__restrict__ X, int64_t ld, int64_t d,
                                                 const int64_t *__restrict__ sel, int m,
                                                 double *__restrict__ mean) {
    extern __shared__ __attribute__((aligned(16))) int64_t srow[];
    if constexpr (SEG) {  // as k_mean's SEG
        const int r0 = (int)blockIdx.y * MEAN_SEG_ROWS;
        sel += r0;
        m = m - r0 < MEAN_SEG_ROWS ? m - r0 : MEAN_SEG_ROWS;
        mean += (int64_t)blockIdx.y * d;
    }
    for (int r = threadIdx.x; r < m; r += 256) srow[r] = sel[r] * ld;
    __syncthreads();
    const double dm = SEG ? 1.0 : (double)m;
    const int64_t nq = (d + 3) >> 2;
    for (int64_t cq = (int64_t)blockIdx.x * 256 + threadIdx.x; cq < nq;
         cq += (int64_t)gridDim.x * 256) {
        const int64_t c = cq * 4;
        if (c + 3 < d) {
            double acc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = ACCUM ? mean[c + e] : 0.0;
            int r = 0;
            for (; r + 8 <= m; r += 8) {
                f4v v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    v[q] = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(X + srow[r + q] + c));
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += (double)v[q][e];
            }
            for (; r < m; ++r) {
                const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(X + srow[r] + c));
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) mean[c + e] = (ACCUM || SEG) ? acc[e] : acc[e] / dm;
        } else {
            for (int64_t cc = c; cc < d; ++cc) {
                double acc = ACCUM ? mean[cc] : 0.0;
                for (int r = 0; r < m; ++r) acc += (double)X[srow[r] + cc];
                mean[cc] = (ACCUM || SEG) ? acc : acc / dm;
            }
        }
    }
}

// the segments of a large selection's K4, in segment order, then / m
__global__ __launch_bounds__(256) void k_mean_comb(const double *__restrict__ part, int S, int64_t d,
                                                   int m, double *__restrict__ mean) {
    const double dm = (double)m;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < d; c += (int64_t)gridDim.x * 256) {
        double acc = 0.0;
        for (int y = 0; y < S; ++y) acc += __builtin_nontemporal_load(part + (int64_t)y * d + c);
        mean[c] = acc / dm;
    }
}

// ---------------------------------------------------------------------------
// synthetic batch: grid (column blocks, rows)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_synth(T *__restrict__ X, int64_t ld, int64_t dl,
                                               int64_t c0, const int64_t *__restrict__ perm,
                                               SynthParams P) {
    const int64_t p = blockIdx.y;
    const int64_t r = perm[p];
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < dl; k += (int64_t)gridDim.x * 256)
        X[p * ld + k] = (T)synth_elem(P, r, c0 + k);
}

// ===========================================================================
// launchers
// ===========================================================================

// fp32 rows whose starts are 16-byte aligned: k_mean_f4 reads 4 columns per load
static bool rows_quad_aligned(const void *X, int dtype, int64_t ld) {
    return dtype != 0 && (ld % 4) == 0 && ((uintptr_t)X % 16) == 0;
}

// One K4 launch: k_mean_f4 over column quads where the rows allow it, else
// k_mean over column pairs (VEC: rows_pair_aligned), at most ~16 blocks per CU.
// SEG: grid y = the selection's segments, each over MEAN_SEG_ROWS row offsets
// in LDS; otherwise all m offsets
template <bool ACCUM, bool SEG>
static hipError_t launch_k4(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *sel,
                            int m, double *out, int num_cu, hipStream_t st) {
    const int S = SEG ? mean_segments(m) : 1;
    const size_t lds = (size_t)(SEG ? MEAN_SEG_ROWS : m) * sizeof(int64_t);
    const int64_t cap = ((int64_t)num_cu * 16 + S - 1) / S;  // 1, 2, 4, 8 per CU: no faster (v13 probe)
    const bool quad = rows_quad_aligned(X, dtype, ld);
    const int64_t per = quad ? 4 : 2;  // columns per thread
    int64_t b = ((d + per - 1) / per + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    const dim3 grid((unsigned)b, (unsigned)S), block(256);
    if (quad)
        hipLaunchKernelGGL((k_mean_f4<ACCUM, SEG>), grid, block, lds, st, (const float *)X, ld, d,
                           sel, m, out);
    else
        with_row_type(dtype, rows_pair_aligned(X, dtype, ld), [&](auto t, auto vec) {
            typedef decltype(t) T;
            hipLaunchKernelGGL((k_mean<T, decltype(vec)::value, ACCUM, SEG>), grid, block, lds, st,
                               (const T *)X, ld, d, sel, m, out);
        });
    return hipGetLastError();
}

hipError_t launch_mean(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *sel, int m,
                       double *mean, int num_cu, hipStream_t st, double *seg_part) {
    const int S = mean_segments(m);
    if (S <= 1 || !seg_part) return launch_k4<false, false>(X, dtype, ld, d, sel, m, mean, num_cu, st);
    // a large selection: the rows in segments of MEAN_SEG_ROWS (grid y), then
    // the segments in order.  A shard's few columns (config E on 8 GPUs: 32,768
    // fp32 columns, 8,192 column threads) left most CUs idle with one thread
    // walking all m rows: 0.25 ms at 1.5 TB/s
    hipError_t e = launch_k4<false, true>(X, dtype, ld, d, sel, m, seg_part, num_cu, st);
    if (e != hipSuccess) return e;
    int64_t b = (d + 255) / 256;
    if (b > (int64_t)num_cu * 8) b = (int64_t)num_cu * 8;
    if (b < 1) b = 1;
    hipLaunchKernelGGL(k_mean_comb, dim3((unsigned)b), dim3(256), 0, st, seg_part, S, d, m, mean);
    return hipGetLastError();
}

hipError_t launch_accumulate(const void *X, int dtype, int64_t ld, int64_t d, const int64_t *idx,
                             int m, double *global, int num_cu, hipStream_t st) {
    return launch_k4<true, false>(X, dtype, ld, d, idx, m, global, num_cu, st);
}

hipError_t launch_synth(void *X, int dtype, int64_t ld, int64_t n, int64_t dl, int64_t c0,
                        const int64_t *perm, const SynthParams &P, hipStream_t st) {
    int64_t bx = (dl + 255) / 256;
    if (bx > 4096) bx = 4096;
    if (bx < 1) bx = 1;
    dim3 grid((unsigned)bx, (unsigned)n), block(256);
    if (dtype == 0)
        hipLaunchKernelGGL(k_synth<double>, grid, block, 0, st, (double *)X, ld, dl, c0, perm, P);
    else
        hipLaunchKernelGGL(k_synth<float>, grid, block, 0, st, (float *)X, ld, dl, c0, perm, P);
    return hipGetLastError();
}

hipError_t configure_mean_kernels() {
    // the masked column sums keep up to BK_MAX_N row offsets in LDS
    for (const void *k : {(const void *)k_mean<double, true, false>,
                          (const void *)k_mean<double, false, false>,
                          (const void *)k_mean<float, true, false>,
                          (const void *)k_mean<float, false, false>,
                          (const void *)k_mean<double, true, true>,
                          (const void *)k_mean<double, false, true>,
                          (const void *)k_mean<float, true, true>,
                          (const void *)k_mean<float, false, true>,
                          (const void *)k_mean_f4<false>, (const void *)k_mean_f4<true>}) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace bk
