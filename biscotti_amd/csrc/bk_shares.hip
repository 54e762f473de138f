// bk_shares.hip -- the secure-aggregation share arithmetic (bk_shares_*,
// DESIGN.md §5u), gfx950.
//
//   k_shares_gen      a client's polynomial shares: the quantised delta cut
//                 into chunks of P coefficients, each evaluated at the T share
//                 points x = s - 10 the way createShareAndWitness does
//                 (DistSys/kyber.go:579-646), bit for bit:
//                     y = sum_j int64(pow(x, j) * float64(c_j))    (wrapping)
//                     y += int64(r),  r the constant term dividePolynomial
//                 (kyber.go:768-793) leaves of the float coefficients with
//                 c_0 replaced by float64(int64(float64(c_0)) - y), divided by
//                 (X - x): the Horner recurrence h <- c_k - (-x) * h in fp64.
//                 The powers are built by fp64 multiplication from x; for
//                 |x| <= 53 and j <= 9 every product is an integer below 2^53,
//                 so they are the exact values a host integer table holds.
//   k_shares_sum      the miner's aggregate (aggregateSecret, kyber.go:244-287):
//                 a gather-sum over the listed slots of the part store,
//                 wrapping int64, 16 bytes per lane (k_qsum's shape).
//   k_shares_recover  the leader's recovery of the integer polynomial of each
//                 chunk (in place of recoverSecret's fp64 least squares,
//                 kyber.go:809-857): Newton divided differences over the first
//                 P points in 128-bit integers, every division exact, expanded
//                 to monomial coefficients and checked modulo 2^64 against all
//                 S points; then updateIntToFloat (kyber.go:745-757) and
//                 global_w + delta (honest.go:408-409) from the same launch.
//
// Built with -ffp-contract=off: every product and difference rounds on its own,
// as Go's amd64 code does.  The per-thread arrays are indexed by unrolled loop
// counters only, so they live in registers (no scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"

namespace bk {

typedef long long i2v __attribute__((ext_vector_type(2)));
typedef __int128 i128;
typedef unsigned __int128 u128;

// Go (amd64) int64(float64), as bk_aggregate.hip's
__device__ __forceinline__ int64_t shares_f64_to_i64(double y) {
    if (y >= -9223372036854775808.0 && y < 9223372036854775808.0) return (int64_t)y;
    return INT64_MIN;
}

// createShareAndWitness's evaluatedValue of the L coefficients cf (float64 of
// the quantised entries) at x
__device__ __forceinline__ int64_t share_value(const double (&cf)[SHARES_MAX_POLY], int L, int x) {
    const double xd = (double)x;
    const double nx = (double)(-x);  // float64(minerSecretX * -1)
    uint64_t y = 0;
    double pw = 1.0;  // math.Pow(x, 0) == 1, also at x == 0
#pragma unroll
    for (int j = 0; j < SHARES_MAX_POLY; ++j) {
        if (j < L) y += (uint64_t)shares_f64_to_i64(pw * cf[j]);
        pw = pw * xd;
    }
    const double c0 = (double)(int64_t)((uint64_t)shares_f64_to_i64(cf[0]) - y);
    // dividePolynomial by (X - x): what it leaves in place 0
    double h = 0.0;
#pragma unroll
    for (int k = SHARES_MAX_POLY - 1; k >= 1; --k)
        if (k < L) h = cf[k] - nx * h;
    h = c0 - nx * h;
    return (int64_t)(y + (uint64_t)shares_f64_to_i64(h * 1.0));
}

__device__ __forceinline__ int load_chunk(const double *__restrict__ delta, int64_t d, double scale,
                                          int P, int64_t chunk, double (&cf)[SHARES_MAX_POLY]) {
    const int64_t e0 = chunk * P;
    const int L = (int)(d - e0 < P ? d - e0 : P);
#pragma unroll
    for (int j = 0; j < SHARES_MAX_POLY; ++j) {
        cf[j] = 0.0;
        if (j < L) cf[j] = (double)shares_f64_to_i64(delta[e0 + j] * scale);
    }
    return L;
}

template <bool PER_CHUNK>
__global__ __launch_bounds__(256) void k_shares_gen(const double *__restrict__ delta, int64_t d,
                                                    int64_t chunks, double scale, int P, int T,
                                                    int64_t *__restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double cf[SHARES_MAX_POLY];
    if constexpr (PER_CHUNK) {
        if (gid >= chunks) return;
        const int L = load_chunk(delta, d, scale, P, gid, cf);
        for (int s = 0; s < T; ++s) y[gid * T + s] = share_value(cf, L, s - SHARES_X0);
    } else {
        if (gid >= chunks * T) return;
        const int64_t chunk = gid / T;
        const int s = (int)(gid - chunk * T);
        const int L = load_chunk(delta, d, scale, P, chunk, cf);
        y[gid] = share_value(cf, L, s - SHARES_X0);
    }
}

__global__ __launch_bounds__(256) void k_shares_sum(const int64_t *__restrict__ store,
                                                    int64_t stride, int64_t elems,
                                                    const int64_t *__restrict__ slots,
                                                    int64_t count, int64_t *__restrict__ out) {
    const int64_t pairs = (elems + 1) / 2;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < pairs;
         u += (int64_t)gridDim.x * 256) {
        const int64_t e = u * 2;
        // the padded row (stride even) makes the pair's second word readable
        // past an odd elems; it is not stored
        uint64_t a0 = 0, a1 = 0;
        int64_t r = 0;
        for (; r + 4 <= count; r += 4) {
            i2v v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                v[q] = *reinterpret_cast<const i2v *>(store + slots[r + q] * stride + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a0 += (uint64_t)v[q].x;
                a1 += (uint64_t)v[q].y;
            }
        }
        for (; r < count; ++r) {
            const i2v v = *reinterpret_cast<const i2v *>(store + slots[r] * stride + e);
            a0 += (uint64_t)v.x;
            a1 += (uint64_t)v.y;
        }
        if (e + 1 < elems) {
            const i2v o = {(long long)a0, (long long)a1};
            *reinterpret_cast<i2v *>(out + e) = o;
        } else {
            out[e] = (int64_t)a0;
        }
    }
}

// a / dv for 1 <= dv < 2^11, by 32-bit limbs (device code has no 128-bit
// division); false: the division leaves a remainder
__device__ __forceinline__ bool div_exact(i128 a, int dv, i128 &q) {
    const bool neg = (a < 0) != (dv < 0);
    const u128 u = a < 0 ? (u128)0 - (u128)a : (u128)a;
    const uint64_t m = (uint64_t)(dv < 0 ? -dv : dv);
    const uint64_t hi = (uint64_t)(u >> 64), lo = (uint64_t)u;
    uint64_t t = hi >> 32;
    const uint64_t q3 = t / m;
    t = ((t - q3 * m) << 32) | (hi & 0xffffffffu);
    const uint64_t q2 = t / m;
    t = ((t - q2 * m) << 32) | (lo >> 32);
    const uint64_t q1 = t / m;
    t = ((t - q1 * m) << 32) | (lo & 0xffffffffu);
    const uint64_t q0 = t / m;
    const u128 uq = ((u128)((q3 << 32) | q2) << 64) | (u128)((q1 << 32) | q0);
    q = neg ? (i128)((u128)0 - uq) : (i128)uq;
    return t - q0 * m == 0;
}

__global__ __launch_bounds__(256) void k_shares_recover(SharesPoints pts, int S, int P, int64_t d,
                                                        int64_t chunks, double scale,
                                                        const double *__restrict__ w,
                                                        int64_t *__restrict__ coef,
                                                        double *__restrict__ delta,
                                                        double *__restrict__ global,
                                                        unsigned long long *__restrict__ bad) {
    constexpr int MP = SHARES_MAX_POLY;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    // Newton's divided differences of the first P points, in place: after
    // level k, dd[i] = f[x_{i-k} .. x_i] for i >= k
    i128 dd[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        dd[i] = 0;
        if (i < P) dd[i] = (i128)pts.base[i][c * pts.stride[i]];
    }
    bool ok = true;
#pragma unroll
    for (int k = 1; k < MP; ++k) {
#pragma unroll
        for (int i = MP - 1; i >= k; --i) {
            if (i < P) {
                i128 q;
                ok &= div_exact(dd[i] - dd[i - 1], pts.x[i] - pts.x[i - k], q);
                dd[i] = q;
            }
        }
    }
    // to monomial coefficients: m <- m * (X - x_k) + dd[k], from the top.
    // |dd[k]| < 2^(64 + k) and |x| <= 53 keep every entry below 2^125
    i128 m[MP];
#pragma unroll
    for (int j = 0; j < MP; ++j) m[j] = 0;
#pragma unroll
    for (int k = MP - 1; k >= 0; --k) {
        if (k < P) {
            const i128 xk = (i128)pts.x[k];
#pragma unroll
            for (int j = MP - 1; j >= 1; --j) m[j] = m[j - 1] - xk * m[j];
            m[0] = dd[k] - xk * m[0];
        }
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) ok &= m[j] == (i128)(int64_t)m[j];
    // every point, modulo 2^64
#pragma unroll
    for (int s = 0; s < SHARES_MAX_POINTS; ++s) {
        if (s < S) {
            const uint64_t x = (uint64_t)(int64_t)pts.x[s];
            uint64_t v = 0;
#pragma unroll
            for (int j = MP - 1; j >= 0; --j) v = v * x + (uint64_t)m[j];
            ok &= v == (uint64_t)pts.base[s][c * pts.stride[s]];
        }
    }
    if (!ok) atomicAdd(bad, 1ull);
    const int64_t e0 = c * P;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        const int64_t e = e0 + j;
        if (j < P && e < d) {
            const int64_t v = ok ? (int64_t)m[j] : 0;
            const double f = (double)v / scale;
            if (coef) coef[e] = v;
            if (delta) delta[e] = f;
            global[e] = w[e] + f;
        }
    }
}

hipError_t launch_shares_gen(const double *delta, int64_t d, double scale, int P, int T,
                             int64_t *y, bool per_chunk, hipStream_t st) {
    const int64_t chunks = (d + P - 1) / P;
    const int64_t threads = per_chunk ? chunks : chunks * T;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (per_chunk)
        hipLaunchKernelGGL(k_shares_gen<true>, grid, block, 0, st, delta, d, chunks, scale, P, T, y);
    else
        hipLaunchKernelGGL(k_shares_gen<false>, grid, block, 0, st, delta, d, chunks, scale, P, T, y);
    return hipGetLastError();
}

hipError_t launch_shares_sum(const int64_t *store, int64_t stride, int64_t elems,
                             const int64_t *slots, int64_t count, int64_t *out, int num_cu,
                             hipStream_t st) {
    int64_t blocks = ((elems + 1) / 2 + 255) / 256;
    const int64_t cap = (int64_t)num_cu * 16;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_shares_sum, dim3((unsigned)blocks), dim3(256), 0, st, store, stride, elems,
                       slots, count, out);
    return hipGetLastError();
}

hipError_t launch_shares_recover(const SharesPoints &pts, int S, int P, int64_t d, double scale,
                                 const double *w, int64_t *coef, double *delta, double *global,
                                 unsigned long long *bad, hipStream_t st) {
    const int64_t chunks = (d + P - 1) / P;
    hipLaunchKernelGGL(k_shares_recover, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st,
                       pts, S, P, d, chunks, scale, w, coef, delta, global, bad);
    return hipGetLastError();
}

}  // namespace bk
