// bk_roni_dev.h -- device helpers the RONI kernels (bk_roni.hip) and the
// evaluation kernels (bk_eval.hip) share: the softmax near-tie test and the
// last-workgroup-out hand-off of a launch's counters.  Included by kernel
// files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"

namespace bk {

// K8's near-tie test (oracle/roni_oracle.c softmax_eval, the same fp64
// expression): the winning logit l1 (class a) and the best other l2 can swap
// under torch's fp32 sgemm rounding only if
//     !( l1 - l2 - u (|l1| + |l2|)  >  E_a + max_c E_c ),  E_c = g (|x| |w_c| + |b_c|)
// (g = gamma_{d_in + 1}(2^-24) (1 + 2^-10), host-computed), or a logit is not
// finite.  xn = |x| of the sample, wn / b the model's C weight-row norms and
// biases (fp32 values), all fp64.
__device__ inline bool softmax_near_tie(const float *lg, int C, int best, double xn,
                                        const double *wn, const double *b, double g) {
    double wmax = 0.0, bmax = 0.0, l2 = -__builtin_inf();
    bool fin = true;
    for (int c = 0; c < C; ++c) {
        const double w = wn[c], ab = __builtin_fabs(b[c]), v = (double)lg[c];
        wmax = w > wmax ? w : wmax;
        bmax = ab > bmax ? ab : bmax;
        fin = fin && __builtin_isfinite(v);
        if (c != best && v > l2) l2 = v;
    }
    const double u = 0x1p-24, l1 = (double)lg[best];
    const double ea = g * (xn * wn[best] + __builtin_fabs(b[best]));
    const double emax = g * (xn * wmax + bmax);
    return !fin || !(l1 - l2 - u * (__builtin_fabs(l1) + __builtin_fabs(l2)) > ea + emax);
}

// The tail of a launch whose workgroups add counts to a zeroed block of
// counters: thread 0 adds the workgroup's counts (agent-scope atomics), drains
// them (vmcnt 0) and adds 1 to the exit counter; the workgroup whose add
// returns gridDim.x - 1 may then read the totals (round_load).  Nobody waits
// for anybody.
constexpr int ROUND_EXIT = 2 * RONI_ROUND_G;
static_assert(ROUND_EXIT < ROUND_CNT_WORDS, "the exit counter lies in the block");

__device__ inline unsigned int round_load(const unsigned int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0 of every workgroup, after the barrier behind the LDS counts: true
// for the last workgroup out, which may then read every workgroup's adds
template <int NC>
__device__ inline bool round_exit(const unsigned int (&s_cnt)[NC], const int (&slot)[NC],
                                  unsigned int *cnt, int exit_slot = ROUND_EXIT) {
#pragma unroll
    for (int q = 0; q < NC; ++q)
        if (s_cnt[q])
            __hip_atomic_fetch_add(cnt + slot[q], s_cnt[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(cnt + exit_slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
           gridDim.x - 1u;
}

}  // namespace bk
