// bk_commit_points.hip -- the miner's G1 point sums (bk_commit_points_*,
// DESIGN.md §5x), gfx950.  The arithmetic is bk_bn256.h's; the point moves are
// bk_commit_dev.h's.
//
// A part is what one client sent this miner (aggregateSecret,
// DistSys/kyber.go:244-287): its CommitmentUpdate, every chunk's Commitment and
// the `held` Witnesses of each chunk the miner keeps.  The store holds one row of
// NP = 1 + chunks (1 + held) points per part, in the order: the update's
// commitment, then per chunk its commitment followed by its witnesses.  A stored
// point is affine, in Montgomery form, 16 words on a 64-byte boundary; infinity
// is (0, 0).
//
//   k_commit_points_in   at bk_commit_points_add: one thread per point of the
//                 arriving part reads its 64 bytes from whichever of the three
//                 arrays the point index falls in, unmarshals and validates it
//                 (a coordinate >= p or a point off the curve leaves the
//                 smallest such index in *bad) and stores the 16 words.
//   k_commit_points_sum<G>   the sum over the listed slots of every point index.
//                 A workgroup owns 256 / G consecutive point indices, G lanes
//                 each.  Gather: lane g of a group takes the list entries j = g
//                 (mod G); the next entry's 64 bytes are on their way while the
//                 current one is added (jac_add_aff, complete).  Combine: the G
//                 partial sums meet across lanes of the wave by the butterfly
//                 xor G/2 .. 1 of complete additions; no LDS, no barrier.
//                 Lane 0 of a group inverts z (one Fermat inversion per point
//                 number), forms x / z^2, y / z^3 and marshals.  One inversion
//                 per workgroup through a product tree in LDS was built and
//                 measured behind this form at every shape.
//
// The sum of a set of points does not depend on the order of the additions, so
// the 64 bytes are the same for every G and every order of the list.  Integer
// arithmetic only; the per-thread arrays are indexed by unrolled counters only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_commit_dev.h"
#include "bk_ctx.h"

namespace bk {

// The 64 bytes of point k of a part in its three arrays (null: not wanted)
template <typename B>
__device__ __forceinline__ B *points_at(int64_t k, int held, B *commit, B *chunk, B *witness) {
    if (k == 0) return commit;
    const int64_t kk = k - 1, c = kk / (held + 1);
    const int r = (int)(kk - c * (held + 1));
    if (r == 0) return chunk ? chunk + c * 64 : nullptr;
    return witness ? witness + (c * held + (r - 1)) * 64 : nullptr;
}

__global__ __launch_bounds__(COMMIT_WG) void k_commit_points_in(
    const uint8_t *__restrict__ commit, const uint8_t *__restrict__ chunk,
    const uint8_t *__restrict__ witness, int held, int64_t np, uint32_t *__restrict__ row,
    unsigned long long *__restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * COMMIT_WG + threadIdx.x;
    if (k >= np) return;
    const uint8_t *src = points_at(k, held, commit, chunk, witness);  // any alignment
    uint8_t raw[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) raw[i] = src[i];
    Aff p;
    if (!aff_unmarshal(raw, &p)) {
        atomicMin(bad, (unsigned long long)k);
        return;
    }
    store_aff(row + k * AFF_WORDS, p);
}

struct PointWords {
    uint4 a, b, c, d;
};

__device__ __forceinline__ Aff aff_of(const PointWords &w) {
    Aff r;
    r.x.v[0] = w.a.x, r.x.v[1] = w.a.y, r.x.v[2] = w.a.z, r.x.v[3] = w.a.w;
    r.x.v[4] = w.b.x, r.x.v[5] = w.b.y, r.x.v[6] = w.b.z, r.x.v[7] = w.b.w;
    r.y.v[0] = w.c.x, r.y.v[1] = w.c.y, r.y.v[2] = w.c.z, r.y.v[3] = w.c.w;
    r.y.v[4] = w.d.x, r.y.v[5] = w.d.y, r.y.v[6] = w.d.z, r.y.v[7] = w.d.w;
    return r;
}

// Round `it` of the gather: the group's G list entries are read by the whole
// wave alike (scalar loads), lane g keeps its own and issues its point's loads
template <int G>
__device__ __forceinline__ bool points_fetch(const uint32_t *__restrict__ col, int64_t stride,
                                             const int64_t *__restrict__ slots, int64_t count,
                                             int64_t it, int g, bool live, PointWords &w) {
    int64_t slot = 0;
#pragma unroll
    for (int q = 0; q < G; ++q) {
        const int64_t j = it * G + q;
        const int64_t s = j < count ? slots[j] : 0;
        slot = q == g ? s : slot;
    }
    const bool have = live && it * G + g < count;
    if (have) {
        const uint4 *v = reinterpret_cast<const uint4 *>(col + slot * stride);
        w.a = v[0], w.b = v[1], w.c = v[2], w.d = v[3];
    }
    return have;
}

template <int G>
__global__ __launch_bounds__(COMMIT_WG) void k_commit_points_sum(
    const uint32_t *__restrict__ store, int64_t stride, int64_t np, int held,
    const int64_t *__restrict__ slots, int64_t count, uint8_t *__restrict__ commit_out,
    uint8_t *__restrict__ chunk_out, uint8_t *__restrict__ witness_out) {
    constexpr int PW = COMMIT_WG / G;  // the point indices of a workgroup
    const int tid = threadIdx.x;
    const int p = tid / G, g = tid % G;
    const int64_t k = (int64_t)blockIdx.x * PW + p;
    const bool live = k < np;
    const uint32_t *col = store + (live ? k : 0) * AFF_WORDS;

    // gather: this lane's share of the list, one point in flight behind the addition
    Jac acc = jac_inf();
    const int64_t rounds = (count + G - 1) / G;
    PointWords nx;
    bool have = points_fetch<G>(col, stride, slots, count, 0, g, live, nx);
#pragma unroll 1
    for (int64_t it = 0; it < rounds; ++it) {
        const PointWords cur = nx;
        const bool had = have;
        have = it + 1 < rounds && points_fetch<G>(col, stride, slots, count, it + 1, g, live, nx);
        if (had) acc = jac_add_aff(acc, aff_of(cur));
    }

    // combine: every lane of the group ends with the group's sum
#pragma unroll 1
    for (int s = G / 2; s >= 1; s >>= 1) {
        Jac o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            o.x.v[i] = __shfl_xor(acc.x.v[i], s);
            o.y.v[i] = __shfl_xor(acc.y.v[i], s);
            o.z.v[i] = __shfl_xor(acc.z.v[i], s);
        }
        acc = jac_add(acc, o);
    }

    const bool inf = !live || jac_is_inf(acc);
    if (g != 0 || !live) return;
    uint8_t *out = points_at(k, held, commit_out, chunk_out, witness_out);
    if (!out) return;
    Aff f = aff_inf();
    if (!inf) {
        const Fp zi = fp_inv(acc.z), zi2 = fp_sqr(zi);
        f.x = fp_mul(acc.x, zi2);
        f.y = fp_mul(fp_mul(acc.y, zi), zi2);
    }
    marshal_aff(f, out);
}

hipError_t launch_commit_points_in(const uint8_t *commit, const uint8_t *chunk,
                                   const uint8_t *witness, int held, int64_t np, uint32_t *row,
                                   unsigned long long *bad, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_points_in, dim3((unsigned)((np + COMMIT_WG - 1) / COMMIT_WG)),
                       dim3(COMMIT_WG), 0, st, commit, chunk, witness, held, np, row, bad);
    return hipGetLastError();
}

// The lane-group width when the caller leaves it to the library: the widest G
// <= count whose grid still fits the device in one pass, COMMIT_POINTS_WG_PER_CU
// workgroups per CU
int commit_points_lanes(int64_t np, int64_t count, int num_cu) {
    const int64_t cap = (int64_t)num_cu * COMMIT_POINTS_WG_PER_CU;
    int g = 1;
    for (int t = 2; t <= COMMIT_POINTS_AUTO_LANES; t *= 2)
        if (t <= count && (np * t + COMMIT_WG - 1) / COMMIT_WG <= cap) g = t;
    return g;
}

hipError_t launch_commit_points_sum(const uint32_t *store, int64_t np, int held,
                                    const int64_t *slots, int64_t count, int lanes,
                                    uint8_t *commit_out, uint8_t *chunk_out, uint8_t *witness_out,
                                    hipStream_t st) {
    const int64_t stride = np * AFF_WORDS;
    const dim3 grid((unsigned)((np * lanes + COMMIT_WG - 1) / COMMIT_WG));
#define BK_POINTS_SUM(G)                                                                       \
    case G:                                                                                    \
        hipLaunchKernelGGL(k_commit_points_sum<G>, grid, dim3(COMMIT_WG), 0, st, store, stride, \
                           np, held, slots, count, commit_out, chunk_out, witness_out);        \
        break;
    switch (lanes) {
        BK_POINTS_SUM(1)
        BK_POINTS_SUM(2)
        BK_POINTS_SUM(4)
        BK_POINTS_SUM(8)
        BK_POINTS_SUM(16)
        default:
            return hipErrorInvalidValue;
    }
#undef BK_POINTS_SUM
    return hipGetLastError();
}

}  // namespace bk
