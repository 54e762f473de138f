// bk_collect_noise.hip -- k_collect_noise: the noise of bk_collect_add_noised
// (include/bk.h), K6's arithmetic on rows that are separate allocations.
//
// One launch noises up to COLLECT_NOISE_ROWS arriving rows of the collection's
// row store over the columns [c0, c1):
//     out_r[c] = delta_r[c] + ((0 + v_r0[c]) + v_r1[c] + ... + v_r(k-1)[c]) / k
// fp64, j ascending, no contraction (the build's -ffp-contract=off): the bits
// of k_noise (bk_aggregate.hip), whose strided layout these rows do not have.
// delta_r is the caller's device row, or the store row itself where the delta
// was uploaded there (in place: every element is read and written by one
// thread).  The k vectors of row r come
//   TAB   through a pointer table in device memory (BK_DEVICE: the caller's
//         rows, read where they are), vector j at tab[r k + j];
//   else  from the collection's staging block (host rows, uploaded there),
//         vector j at stage + (r k + j) sld, its column c at [c - c0].
// A pair of columns per lane: 16-byte non-temporal loads where the vector is
// 16-B aligned (c0 is even, so the base decides -- wave-uniform), two 8-byte
// loads where a BK_DEVICE row is not; the store row is 16-B aligned, so a whole
// pair leaves as one 16-byte non-temporal store.  The last column of an odd d
// goes alone, 8 bytes: the pad columns [d, ld) of the store row are never
// written (k_border reads them as zeros).  Eight loads in flight over j, as
// k_noise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"

namespace bk {

namespace {

typedef double nd2 __attribute__((ext_vector_type(2)));

// columns c, c + 1 of a row whose base is p - c (c even: p is 16-B aligned iff
// the base is)
__device__ __forceinline__ nd2 ld_pair(const double *p) {
    if (((uintptr_t)p & 15) == 0) return __builtin_nontemporal_load(reinterpret_cast<const nd2 *>(p));
    nd2 v;
    v.x = __builtin_nontemporal_load(p);
    v.y = __builtin_nontemporal_load(p + 1);
    return v;
}

// grid (column blocks, rows), 256 threads; the column pairs grid-strided
template <bool TAB>
__global__ __launch_bounds__(256) void k_collect_noise(const CollectNoiseArgs a) {
    const int r = (int)blockIdx.y;
    const int k = a.k;
    const double dk = (double)k;
    const double *delta = a.delta[r];
    double *out = a.out[r];
    const double *const *tab = TAB ? a.tab + (int64_t)r * k : nullptr;
    // vector j's element of column c at vec(j)[c - off]
    const double *stage = TAB ? nullptr : a.stage + (int64_t)r * k * a.sld;
    const int64_t off = TAB ? 0 : a.c0;
    const auto vec = [&](int j) -> const double * {
        if constexpr (TAB)
            return tab[j];
        else
            return stage + (int64_t)j * a.sld;
    };
    const int64_t npair = (a.c1 - a.c0 + 1) >> 1;
    for (int64_t cp = (int64_t)blockIdx.x * 256 + threadIdx.x; cp < npair;
         cp += (int64_t)gridDim.x * 256) {
        const int64_t c = a.c0 + cp * 2;
        if (c + 1 < a.c1) {
            nd2 s = {0.0, 0.0};
            int j = 0;
            for (; j + 8 <= k; j += 8) {
                nd2 v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = ld_pair(vec(j + q) + (c - off));
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    s.x += v[q].x;
                    s.y += v[q].y;
                }
            }
            for (; j < k; ++j) {
                const nd2 v = ld_pair(vec(j) + (c - off));
                s.x += v.x;
                s.y += v.y;
            }
            const nd2 x = ld_pair(delta + c);
            nd2 o;
            o.x = x.x + s.x / dk;
            o.y = x.y + s.y / dk;
            __builtin_nontemporal_store(o, reinterpret_cast<nd2 *>(out + c));
        } else {  // the last column of an odd d
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += __builtin_nontemporal_load(vec(j) + (c - off));
            out[c] = delta[c] + s / dk;
        }
    }
}

}  // namespace

hipError_t launch_collect_noise(const CollectNoiseArgs &a, int num_cu, hipStream_t st) {
    const int64_t npair = (a.c1 - a.c0 + 1) / 2;
    int64_t bx = (npair + 255) / 256;
    // a few waves of blocks over the chip, the rest of a row grid-strided
    const int64_t cap = ((int64_t)num_cu * 16 + a.rows - 1) / a.rows;
    if (bx > cap) bx = cap;
    if (bx < 1) bx = 1;
    const dim3 grid((unsigned)bx, (unsigned)a.rows), block(256);
    if (a.tab)
        hipLaunchKernelGGL(k_collect_noise<true>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_collect_noise<false>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace bk
