// bk_commit.hip -- the polynomial commitments in bn256 G1 (bk_commit_*,
// DESIGN.md §5w), gfx950.  The arithmetic is bk_bn256.h's.
//
//   k_commit_key      at bk_commit_set_key: one thread per key point unmarshals
//                 and validates it (a coordinate >= p or a point off the curve
//                 leaves the smallest such index in *bad) and stores its
//                 multiples 1 .. 8, affine, in Montgomery form: 512 bytes per
//                 point, what a signed 4-bit window needs.
//   k_commit_msm      createCommitment (DistSys/kyber.go:533-562): sum v_i
//                 PK[first + i].  SetInt64(v) is v mod n, so v P = |v| (-P): no
//                 scalar has more than 64 bits.  A thread takes the terms i =
//                 its number, + the grid's threads, ...; it walks the 17
//                 windows from the top, four doublings between two windows
//                 shared by all its terms, one mixed addition per non-zero
//                 digit.  While its sum is infinity (the top windows of small
//                 scalars) it doubles nothing.  The workgroup adds its 256 sums
//                 through LDS by the fixed tree (strides 128 .. 1) of complete
//                 additions and stores one Jacobian point; the workgroup that
//                 leaves last adds those by the same tree, converts to affine
//                 and marshals -- bk_grad.hip's hand-off, nobody waits.
//   k_commit_chunks   fillPolynomialMap's commitment (kyber.go:172-202) of every
//                 chunk c of P coefficients over PK[c P + j], j < L (the last
//                 chunk may be shorter): one thread per chunk, the same walk
//                 over its up to 10 terms.
//   k_commit_witness  createShareAndWitness's witness (kyber.go:579-646): one
//                 thread per (chunk, share s).  The quotient's coefficients are
//                 the Horner intermediates of share_value (bk_shares.hip): the
//                 lines marked [share_value] below restate that function's
//                 recurrence h <- c_k - (-x) h, k = L-1 .. 1, x = s - 10, in
//                 fp64, and qInt[k-1] = int64(h) by Go's conversion.  c_0, which
//                 the reference replaces first, enters no quotient coefficient;
//                 the appended trailing 0 adds nothing.  The L-1 terms share
//                 their doublings (Straus).
//
// The result of a sum of points does not depend on the order of the additions:
// the 64 marshalled bytes are those of the reference whatever the grid.  One
// Fermat inversion per output point.  Built with -ffp-contract=off; the
// per-thread arrays are indexed by unrolled counters only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_bn256.h"
#include "bk_ctx.h"

namespace bk {

using namespace bn;

constexpr int COMMIT_WG = 256;
constexpr int JAC_WORDS = 24;  // a Jacobian point: 3 x 8 limbs
constexpr int AFF_WORDS = 16;

// Go (amd64) int64(float64), as bk_shares.hip's
__device__ __forceinline__ int64_t commit_f64_to_i64(double y) {
    if (y >= -9223372036854775808.0 && y < 9223372036854775808.0) return (int64_t)y;
    return INT64_MIN;
}

// entry e of the quantised update: q as given, or int64(delta * 10^precision)
__device__ __forceinline__ int64_t commit_scalar(const double *__restrict__ delta,
                                                 const int64_t *__restrict__ q, double scale,
                                                 int64_t e) {
    return q ? q[e] : commit_f64_to_i64(delta[e] * scale);
}

__device__ __forceinline__ Aff load_aff(const uint32_t *__restrict__ p) {
    const uint4 *v = reinterpret_cast<const uint4 *>(p);
    const uint4 a = v[0], b = v[1], c = v[2], d = v[3];
    Aff r;
    r.x.v[0] = a.x, r.x.v[1] = a.y, r.x.v[2] = a.z, r.x.v[3] = a.w;
    r.x.v[4] = b.x, r.x.v[5] = b.y, r.x.v[6] = b.z, r.x.v[7] = b.w;
    r.y.v[0] = c.x, r.y.v[1] = c.y, r.y.v[2] = c.z, r.y.v[3] = c.w;
    r.y.v[4] = d.x, r.y.v[5] = d.y, r.y.v[6] = d.z, r.y.v[7] = d.w;
    return r;
}

__device__ __forceinline__ void store_aff(uint32_t *p, const Aff &a) {
    uint4 *v = reinterpret_cast<uint4 *>(p);
    v[0] = make_uint4(a.x.v[0], a.x.v[1], a.x.v[2], a.x.v[3]);
    v[1] = make_uint4(a.x.v[4], a.x.v[5], a.x.v[6], a.x.v[7]);
    v[2] = make_uint4(a.y.v[0], a.y.v[1], a.y.v[2], a.y.v[3]);
    v[3] = make_uint4(a.y.v[4], a.y.v[5], a.y.v[6], a.y.v[7]);
}

// a Jacobian point to and from 24 words of LDS or global memory
template <typename T>
__device__ __forceinline__ Jac load_jac(const T *p) {
    Jac r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r.x.v[i] = p[i];
        r.y.v[i] = p[8 + i];
        r.z.v[i] = p[16 + i];
    }
    return r;
}
template <typename T>
__device__ __forceinline__ void store_jac(T *p, const Jac &a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        p[i] = a.x.v[i];
        p[8 + i] = a.y.v[i];
        p[16 + i] = a.z.v[i];
    }
}

// window w of the term v PK[i]: acc += digit (table of PK[i])
__device__ __forceinline__ void add_window(Jac &acc, int64_t v, int w,
                                           const uint32_t *__restrict__ tab) {
    int dg = scalar_digit(scalar_abs(v), w);
    if (dg == 0) return;
    if (v < 0) dg = -dg;
    Aff e = load_aff(tab + (size_t)((dg < 0 ? -dg : dg) - 1) * AFF_WORDS);
    if (dg < 0) e = aff_neg(e);
    acc = jac_add_aff(acc, e);
}

__device__ __forceinline__ void shift_window(Jac &acc) {
    if (jac_is_inf(acc)) return;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) acc = jac_dbl(acc);
}

// the affine point of a, marshalled (64 bytes, any alignment)
__device__ __forceinline__ void marshal_out(const Jac &a, uint8_t *__restrict__ out) {
    const Aff f = jac_to_aff(a);
    const Fp x = fp_from_mont(f.x), y = fp_from_mont(f.y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            out[28 - 4 * i + b] = (uint8_t)(x.v[i] >> (24 - 8 * b));
            out[60 - 4 * i + b] = (uint8_t)(y.v[i] >> (24 - 8 * b));
        }
    }
}

__global__ __launch_bounds__(COMMIT_WG) void k_commit_key(const uint8_t *__restrict__ pk,
                                                          int64_t count,
                                                          uint32_t *__restrict__ table,
                                                          unsigned long long *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * COMMIT_WG + threadIdx.x;
    if (i >= count) return;
    uint8_t raw[64];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(pk + i * 64);  // 64-byte entries of a 256-byte aligned buffer
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t wd = src[k];
        raw[4 * k] = (uint8_t)wd;
        raw[4 * k + 1] = (uint8_t)(wd >> 8);
        raw[4 * k + 2] = (uint8_t)(wd >> 16);
        raw[4 * k + 3] = (uint8_t)(wd >> 24);
    }
    Aff p;
    if (!aff_unmarshal(raw, &p)) {
        atomicMin(bad, (unsigned long long)i);
        p = aff_inf();
    }
    uint32_t *t = table + (size_t)i * TABLE * AFF_WORDS;
    store_aff(t, p);
    Jac acc = jac_from_aff(p);
#pragma unroll 1
    for (int k = 1; k < TABLE; ++k) {
        acc = jac_add_aff(acc, p);
        store_aff(t + k * AFF_WORDS, jac_to_aff(acc));
    }
}

// Behind a workgroup's plain stores of handed-off data: true, in every thread,
// for the workgroup that left last of `total` (bk_grad.hip's grad_last_out)
__device__ inline bool commit_last_out(unsigned int *cnt, unsigned int total, unsigned int *s_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT) == total - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        *s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return *s_last != 0u;
}

__global__ __launch_bounds__(COMMIT_WG) void k_commit_msm(const double *__restrict__ delta,
                                                          const int64_t *__restrict__ q,
                                                          double scale, int64_t n,
                                                          const uint32_t *__restrict__ table,
                                                          uint32_t *__restrict__ part,
                                                          unsigned int *__restrict__ cnt,
                                                          uint8_t *__restrict__ out) {
    __shared__ uint32_t red[COMMIT_WG * JAC_WORDS];
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * COMMIT_WG + tid;
    const int64_t step = (int64_t)gridDim.x * COMMIT_WG;
    Jac acc = jac_inf();
#pragma unroll 1
    for (int w = WINDOWS - 1; w >= 0; --w) {
        shift_window(acc);
#pragma unroll 1
        for (int64_t i = first; i < n; i += step)
            add_window(acc, commit_scalar(delta, q, scale, i), w,
                       table + (size_t)i * TABLE * AFF_WORDS);
    }
    // the workgroup's 256 sums, then the workgroups' sums, by one tree
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
        store_jac(red + tid * JAC_WORDS, acc);
#pragma unroll 1
        for (int s = COMMIT_WG / 2; s >= 1; s >>= 1) {
            __syncthreads();
            if (tid < s) {
                acc = jac_add(acc, load_jac(red + (tid + s) * JAC_WORDS));
                store_jac(red + tid * JAC_WORDS, acc);
            }
        }
        if (phase == 1 || gridDim.x == 1) break;
        if (tid == 0) store_jac(part + (size_t)blockIdx.x * JAC_WORDS, acc);
        if (!commit_last_out(cnt, gridDim.x, &s_last)) return;
        // gridDim.x <= COMMIT_WG (launch_commit_msm)
        acc = tid < (int)gridDim.x ? load_jac(part + (size_t)tid * JAC_WORDS) : jac_inf();
    }
    if (tid == 0) marshal_out(acc, out);
}

// the walk over the up to SHARES_MAX_POLY terms v[j] PK[j], j < L, of one thread
__device__ __forceinline__ Jac commit_few(const int64_t (&v)[SHARES_MAX_POLY], int L,
                                          const uint32_t *__restrict__ table) {
    Jac acc = jac_inf();
#pragma unroll 1
    for (int w = WINDOWS - 1; w >= 0; --w) {
        shift_window(acc);
#pragma unroll 1
        for (int j = 0; j < L; ++j) {
            int64_t vj = 0;
#pragma unroll
            for (int k = 0; k < SHARES_MAX_POLY; ++k) vj = k == j ? v[k] : vj;
            add_window(acc, vj, w, table + (size_t)j * TABLE * AFF_WORDS);
        }
    }
    return acc;
}

__global__ __launch_bounds__(COMMIT_WG) void k_commit_chunks(const double *__restrict__ delta,
                                                             const int64_t *__restrict__ q,
                                                             double scale, int64_t d,
                                                             int64_t chunks, int P,
                                                             const uint32_t *__restrict__ table,
                                                             uint8_t *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * COMMIT_WG + threadIdx.x;
    if (c >= chunks) return;
    const int64_t e0 = c * P;
    const int L = (int)(d - e0 < P ? d - e0 : P);
    int64_t v[SHARES_MAX_POLY];
#pragma unroll
    for (int j = 0; j < SHARES_MAX_POLY; ++j) v[j] = j < L ? commit_scalar(delta, q, scale, e0 + j) : 0;
    marshal_out(commit_few(v, L, table + (size_t)e0 * TABLE * AFF_WORDS), out + c * 64);
}

__global__ __launch_bounds__(COMMIT_WG) void k_commit_witness(const double *__restrict__ delta,
                                                              const int64_t *__restrict__ q,
                                                              double scale, int64_t d,
                                                              int64_t chunks, int P, int T,
                                                              const uint32_t *__restrict__ table,
                                                              uint8_t *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * COMMIT_WG + threadIdx.x;
    if (gid >= chunks * T) return;
    const int64_t c = gid / T;
    const int s = (int)(gid - c * T);
    const int64_t e0 = c * P;
    const int L = (int)(d - e0 < P ? d - e0 : P);
    double cf[SHARES_MAX_POLY];
#pragma unroll
    for (int j = 0; j < SHARES_MAX_POLY; ++j)
        cf[j] = j < L ? (double)commit_scalar(delta, q, scale, e0 + j) : 0.0;
    const double nx = (double)(-(s - SHARES_X0));  // [share_value] float64(minerSecretX * -1)
    int64_t v[SHARES_MAX_POLY];
    v[SHARES_MAX_POLY - 1] = 0;
    double h = 0.0;  // [share_value]
#pragma unroll
    for (int k = SHARES_MAX_POLY - 1; k >= 1; --k) {  // [share_value]
        if (k < L) h = cf[k] - nx * h;                // [share_value]
        v[k - 1] = k < L ? commit_f64_to_i64(h) : 0;
    }
    marshal_out(commit_few(v, L - 1, table + (size_t)e0 * TABLE * AFF_WORDS), out + gid * 64);
}

hipError_t launch_commit_key(const uint8_t *pk, int64_t count, uint32_t *table,
                             unsigned long long *bad, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_key, dim3((unsigned)((count + COMMIT_WG - 1) / COMMIT_WG)),
                       dim3(COMMIT_WG), 0, st, pk, count, table, bad);
    return hipGetLastError();
}

int commit_msm_groups(int64_t n, int terms) {
    const int64_t threads = (n + terms - 1) / terms;
    int64_t g = (threads + COMMIT_WG - 1) / COMMIT_WG;
    if (g > COMMIT_MAX_GROUPS) g = COMMIT_MAX_GROUPS;
    return (int)(g < 1 ? 1 : g);
}

hipError_t launch_commit_msm(const double *delta, const int64_t *q, double scale, int64_t n,
                             const uint32_t *table, uint32_t *part, unsigned int *cnt,
                             uint8_t *out, int terms, hipStream_t st) {
    static_assert(COMMIT_MAX_GROUPS <= COMMIT_WG, "the last workgroup takes one sum per thread");
    hipLaunchKernelGGL(k_commit_msm, dim3((unsigned)commit_msm_groups(n, terms)), dim3(COMMIT_WG), 0,
                       st, delta, q, scale, n, table, part, cnt, out);
    return hipGetLastError();
}

hipError_t launch_commit_chunks(const double *delta, const int64_t *q, double scale, int64_t d,
                                int P, const uint32_t *table, uint8_t *out, hipStream_t st) {
    const int64_t chunks = (d + P - 1) / P;
    hipLaunchKernelGGL(k_commit_chunks, dim3((unsigned)((chunks + COMMIT_WG - 1) / COMMIT_WG)),
                       dim3(COMMIT_WG), 0, st, delta, q, scale, d, chunks, P, table, out);
    return hipGetLastError();
}

hipError_t launch_commit_witness(const double *delta, const int64_t *q, double scale, int64_t d,
                                 int P, int T, const uint32_t *table, uint8_t *out,
                                 hipStream_t st) {
    const int64_t chunks = (d + P - 1) / P;
    hipLaunchKernelGGL(k_commit_witness,
                       dim3((unsigned)((chunks * T + COMMIT_WG - 1) / COMMIT_WG)), dim3(COMMIT_WG), 0,
                       st, delta, q, scale, d, chunks, P, T, table, out);
    return hipGetLastError();
}

}  // namespace bk
