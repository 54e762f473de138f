// bk_block.hip -- the miner's block aggregation as the updates arrive
// (bk_block_*), gfx950.
//
//   k_block_add<T, Q, FIN>   the rows of one launch group (up to BLOCK_GROUP
//                 arrivals) added to the running gradient in arrival order:
//                     gout[c] = ((gin[c] + row_0[c]) + row_1[c]) + ...
//                 sequential fp64 adds, the bits of the loop of
//                 Honest.createBlock (DistSys/honest.go:361-375) and of K4's
//                 ACCUM variant (bk_mean.hip) over the same rows.
//                 Q: the secure path's running sum next to it, from the same
//                 loaded value: qout[c] = qin[c] + sum_r int64(row_r[c] * 10^p),
//                 wrapping (k_qsum's arithmetic, bk_aggregate.hip).
//                 FIN: the new gradient (and q, q / 10^p) also stored into the
//                 block's mapped host output, so the finish is the stream wait.
//
// One pass, no hand-offs between workgroups and no atomics: a thread owns 16
// bytes of every row's columns, reads gin / qin, writes gout / qout (another
// buffer: the host swaps the two once the launch is queued, so a launch that
// fails leaves the block as it was).  The row pointers and the mask of
// accepted rows travel in the launch arguments.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"

namespace bk {

typedef double d2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

// Go (amd64) int64(float64), as bk_aggregate.hip's
__device__ __forceinline__ int64_t block_f64_to_i64(double y) {
    if (y >= -9223372036854775808.0 && y < 9223372036854775808.0) return (int64_t)y;
    return INT64_MIN;
}

template <typename T>
__device__ __forceinline__ T ldnt1(const T *p) {
#ifndef BK_NO_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// the W = 16 / sizeof(T) columns from c on of one row, widened; al: the row
// starts on a 16-byte boundary (one 16-byte load), else element loads
template <typename T>
struct RowLoad;
template <>
struct RowLoad<double> {
    static constexpr int W = 2;
    __device__ static __forceinline__ void ld(const double *p, bool al, double (&v)[2]) {
        if (al) {
            const d2v t = ldnt1(reinterpret_cast<const d2v *>(p));
            v[0] = t.x;
            v[1] = t.y;
        } else {
            v[0] = ldnt1(p);
            v[1] = ldnt1(p + 1);
        }
    }
};
template <>
struct RowLoad<float> {
    static constexpr int W = 4;
    __device__ static __forceinline__ void ld(const float *p, bool al, double (&v)[4]) {
        if (al) {
            const f4v t = ldnt1(reinterpret_cast<const f4v *>(p));
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (double)t[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (double)ldnt1(p + e);
        }
    }
};

// rows.p[i]: arrival i of the group; bit i of acc: it is accepted (a rejected
// row's pointer is never read); bit i of al: it is 16-byte aligned
template <typename T, bool Q, bool FIN>
__global__ __launch_bounds__(256) void k_block_add(BlockRows rows, unsigned acc, unsigned al,
                                                   int64_t d, const double *__restrict__ gin,
                                                   double *__restrict__ gout,
                                                   const int64_t *__restrict__ qin,
                                                   int64_t *__restrict__ qout, double scale,
                                                   double *__restrict__ hg,
                                                   int64_t *__restrict__ hq,
                                                   double *__restrict__ hqf) {
    constexpr int W = RowLoad<T>::W;
    const int64_t units = (d + W - 1) / W;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units;
         u += (int64_t)gridDim.x * 256) {
        const int64_t c = u * W;
        if (c + W <= d) {
            double g[W];
            uint64_t q[W];
            double v[BLOCK_GROUP][W];
#pragma unroll
            for (int r = 0; r < BLOCK_GROUP; ++r)
                if (acc >> r & 1) RowLoad<T>::ld((const T *)rows.p[r] + c, al >> r & 1, v[r]);
#pragma unroll
            for (int e = 0; e < W; e += 2) {
                const d2v t = *reinterpret_cast<const d2v *>(gin + c + e);
                g[e] = t.x;
                g[e + 1] = t.y;
                if constexpr (Q) {
                    q[e] = (uint64_t)qin[c + e];
                    q[e + 1] = (uint64_t)qin[c + e + 1];
                }
            }
#pragma unroll
            for (int r = 0; r < BLOCK_GROUP; ++r)
                if (acc >> r & 1) {
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        g[e] = g[e] + v[r][e];
                        if constexpr (Q) q[e] += (uint64_t)block_f64_to_i64(v[r][e] * scale);
                    }
                }
#pragma unroll
            for (int e = 0; e < W; e += 2) {
                const d2v t = {g[e], g[e + 1]};
                *reinterpret_cast<d2v *>(gout + c + e) = t;
                if constexpr (FIN) *reinterpret_cast<d2v *>(hg + c + e) = t;
            }
            if constexpr (Q) {
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    qout[c + e] = (int64_t)q[e];
                    if constexpr (FIN) {
                        hq[c + e] = (int64_t)q[e];
                        hqf[c + e] = (double)(int64_t)q[e] / scale;
                    }
                }
            }
        } else {
            // the last columns of a d that is no multiple of W
            for (int64_t cc = c; cc < d; ++cc) {
                double g = gin[cc];
                uint64_t q = 0;
                if constexpr (Q) q = (uint64_t)qin[cc];
                for (int r = 0; r < BLOCK_GROUP; ++r)
                    if (acc >> r & 1) {
                        const double x = (double)ldnt1((const T *)rows.p[r] + cc);
                        g = g + x;
                        if constexpr (Q) q += (uint64_t)block_f64_to_i64(x * scale);
                    }
                gout[cc] = g;
                if constexpr (FIN) hg[cc] = g;
                if constexpr (Q) {
                    qout[cc] = (int64_t)q;
                    if constexpr (FIN) {
                        hq[cc] = (int64_t)q;
                        hqf[cc] = (double)(int64_t)q / scale;
                    }
                }
            }
        }
    }
}

template <typename T>
static hipError_t launch_block_t(const BlockLaunch &L, int num_cu, hipStream_t st) {
    constexpr int W = RowLoad<T>::W;
    const int64_t units = (L.d + W - 1) / W;
    int64_t blocks = (units + 255) / 256;
    const int64_t cap = (int64_t)num_cu * 16;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    unsigned al = 0;
    for (int r = 0; r < BLOCK_GROUP; ++r)
        if ((L.acc >> r & 1) && ((uintptr_t)L.rows.p[r] % 16) == 0) al |= 1u << r;
    const dim3 grid((unsigned)blocks), block(256);
    const bool q = L.qin != nullptr;
#define BK_BLOCK_GO(Q, FIN)                                                                    \
    hipLaunchKernelGGL((k_block_add<T, Q, FIN>), grid, block, 0, st, L.rows, L.acc, al, L.d,   \
                       L.gin, L.gout, L.qin, L.qout, L.scale, L.hg, L.hq, L.hqf)
    if (q && L.fin)
        BK_BLOCK_GO(true, true);
    else if (q)
        BK_BLOCK_GO(true, false);
    else if (L.fin)
        BK_BLOCK_GO(false, true);
    else
        BK_BLOCK_GO(false, false);
#undef BK_BLOCK_GO
    return hipGetLastError();
}

hipError_t launch_block_add(const BlockLaunch &L, int num_cu, hipStream_t st) {
    return L.dtype == 0 ? launch_block_t<double>(L, num_cu, st) : launch_block_t<float>(L, num_cu, st);
}

}  // namespace bk
