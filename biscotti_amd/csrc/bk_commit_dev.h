// bk_commit_dev.h -- what the G1 kernels share (bk_commit.hip, DESIGN.md §5w;
// bk_commit_points.hip, §5x): a point to and from registers, LDS and global
// memory, and the marshalled bytes.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_bn256.h"

namespace bk {

using namespace bn;

constexpr int COMMIT_WG = 256;
constexpr int JAC_WORDS = 24;  // a Jacobian point: 3 x 8 limbs
constexpr int AFF_WORDS = 16;

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

// the affine point f (Montgomery form), marshalled (64 bytes, any alignment)
__device__ __forceinline__ void marshal_aff(const Aff &f, uint8_t *__restrict__ out) {
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

// the affine point of a, marshalled
__device__ __forceinline__ void marshal_out(const Jac &a, uint8_t *__restrict__ out) {
    marshal_aff(jac_to_aff(a), out);
}

}  // namespace bk
