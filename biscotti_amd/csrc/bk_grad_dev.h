// bk_grad_dev.h -- device helpers the gradient kernels share (bk_grad.hip,
// bk_grad_cnn.hip): the quantisation rule, the last arriver's hand-off and the
// fixed tree of 256 values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_ctx.h"

namespace bk {

// Go (amd64) int64(float64), k_qsum's rule: truncation; NaN and values outside
// [-2^63, 2^63) give 0x8000000000000000
__device__ __forceinline__ int64_t grad_i64(double y) {
    if (y >= -9223372036854775808.0 && y < 9223372036854775808.0) return (int64_t)y;
    return INT64_MIN;
}

// Behind a workgroup's plain stores of handed-off data: true, in every thread,
// for the workgroup that left last of `total`; its loads then see every other
// workgroup's stores.  It puts the counter back to zero for the next launch
__device__ inline bool grad_last_out(unsigned int *cnt, unsigned int total, unsigned int *s_last) {
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

// red[0] = the 256 values' sum by the fixed tree (strides 128, 64, .. 1)
__device__ inline double grad_tree(double *red, double v) {
    const int tid = threadIdx.x;
    __syncthreads();  // red's previous use is over
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = GRAD_TILE / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

}  // namespace bk
