// bk_gram.hip -- the Gram stages of the Multi-Krum engine, CDNA4 (gfx950).
//
// The first two steps of one Multi-Krum call (DESIGN.md "Kernels"; the later
// ones are in bk_scores.hip and bk_mean.hip):
//   K1  k_gram      split-K, upper-triangle fp64 Gram partials on
//                   v_mfma_f64_16x16x4_f64 (the -2XX^T term of
//                   logistic_validator.py:59-60; norms come from its diagonal)
//       k_gram3     the same from a workgroup-shared LDS ring (K1 v3: rows with
//                   16-byte aligned starts, the headline path)
//   K1b k_reduce    fixed-order sum of the split-K partials -> packed upper
//       k_reduce3   (k_gram3's slabs)
// and the packed upper's fixed-order sums across column chunks (k_add_upper)
// and ranks (k_sum_ranks).
//
// Built with -ffp-contract=off: every non-MFMA add/mul rounds exactly as the
// numpy reference evaluates it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bk_device.h"
#include "bk_internal.h"

namespace bk {

// ---------------------------------------------------------------------------
// K1: split-K upper-triangle Gram on fp64 MFMA.
//
// One WAVE owns one task = (64x64 upper sub-tile u, k-piece s).  No LDS, no
// barriers: fp64 MFMA is 64 cycles per 16x16x4 on gfx950, so a wave's 16
// accumulators hide everything if operands arrive from a register ring P
// k-blocks deep.  The contraction index is permuted inside each 8-column
// k-block so that every lane loads 16 contiguous bytes per row:
//   lane l (rr = l&15, g = l>>4) holds X[row rr][kb*8 + 2g + s] for MFMA
//   sub-step s in {0,1}; A and B use the same permutation, so the product is
//   exactly X X^T (the order of the k-sum is a free choice, as in any BLAS).
// Output: acc[a][b] is the 16x16 block (a,b) of the sub-tile; element
// (row g + 4r, col rr) sits in register r (f64 MFMA C/D map,
// cdna_hip_programming.md §3).
// ---------------------------------------------------------------------------

template <typename T, bool VEC, bool DIAG>
__device__ __forceinline__ void gram_load(const T *(&pa)[4], const T *(&pb)[4],
                                          int64_t off, d2v (&a)[4], d2v (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = ld2<T, VEC>(pa[i] + off);
    if constexpr (!DIAG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = ld2<T, VEC>(pb[j] + off);
    }
}

template <bool DIAG>
__device__ __forceinline__ void gram_mma(d4v (&acc)[4][4], const d2v (&a)[4], const d2v (&b)[4]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (DIAG && j < i) continue;
                const double bv = DIAG ? a[j][s] : b[j][s];
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][s], bv, acc[i][j], 0, 0, 0);
            }
        }
    }
}

template <typename T, bool VEC, bool DIAG, int P>
__device__ __forceinline__ void gram_task(const T *__restrict__ X, int64_t ld, int n, int rowA,
                                          int rowB, int64_t k0, int64_t k1, d4v (&acc)[4][4]) {
    const int lane = threadIdx.x & 63, rr = lane & 15, g = lane >> 4;
    const T *pa[4];
    const T *pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = min(rowA + i * 16 + rr, n - 1);
        pa[i] = X + (int64_t)ra * ld + k0 + 2 * g;
        const int rb = min(rowB + i * 16 + rr, n - 1);
        pb[i] = X + (int64_t)rb * ld + k0 + 2 * g;
    }
    const int64_t len = k1 - k0;
    const int64_t nb = len >> 3;
    const int64_t rem = nb % P;

    // (1) the first nb % P blocks, unpipelined, so the ring runs a multiple of P
    for (int64_t kb = 0; kb < rem; ++kb) {
        d2v a[4], b[4];
        gram_load<T, VEC, DIAG>(pa, pb, kb * 8, a, b);
        gram_mma<DIAG>(acc, a, b);
    }
    // (2) register ring, P k-blocks in flight
    if (nb > rem) {
        d2v ra[P][4], rb[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            gram_load<T, VEC, DIAG>(pa, pb, (rem + p) * 8, ra[p], rb[p]);
            __builtin_amdgcn_sched_barrier(0);  // issue stages in ring order
        }
        for (int64_t kb = rem; kb < nb; kb += P) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                gram_mma<DIAG>(acc, ra[p], rb[p]);
                int64_t nk = kb + P + p;
                nk = nk < nb ? nk : nb - 1;  // clamped re-load past the end keeps waits static
                gram_load<T, VEC, DIAG>(pa, pb, nk * 8, ra[p], rb[p]);
                // keep the prefetch here: without the fence the scheduler sinks it to
                // the top of the next trip and the ring degenerates to load-then-wait
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // (3) ragged tail: len % 8 columns, guarded scalar loads
    if (len & 7) {
        const int64_t kt = nb * 8;
        d2v a[4], b[4];
        const bool v0 = kt + 2 * g < len, v1 = kt + 2 * g + 1 < len;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i].x = v0 ? (double)pa[i][kt] : 0.0;
            a[i].y = v1 ? (double)pa[i][kt + 1] : 0.0;
            b[i].x = v0 ? (double)pb[i][kt] : 0.0;
            b[i].y = v1 ? (double)pb[i][kt + 1] : 0.0;
        }
        gram_mma<DIAG>(acc, a, b);
    }
}

template <typename T, bool VEC, int P>
__global__ __launch_bounds__(256, 1) void k_gram(const T *__restrict__ X, int64_t ld, int n,
                                                 int64_t d, int T_, int ntile, int S, int64_t kc,
                                                 int nwg, double *__restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lwg = xcd_remap(blockIdx.x, nwg);
    const int task = lwg * 4 + wave;  // tasks are piece-major: task = s*ntile + u
    if (task >= ntile * S) return;    // wave-uniform
    const int s = task / ntile, u = task - s * ntile;
    int bi, bj;
    tri_decode(u, T_, bi, bj);
    const int64_t k0 = (int64_t)s * kc;
    const int64_t k1 = min(d, k0 + kc);

    d4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = d4v{0.0, 0.0, 0.0, 0.0};

    if (k1 > k0) {
        if (bi == bj)
            gram_task<T, VEC, true, P>(X, ld, n, bi * 64, bj * 64, k0, k1, acc);
        else
            gram_task<T, VEC, false, P>(X, ld, n, bi * 64, bj * 64, k0, k1, acc);
    }

    double *out = part + (int64_t)task * 4096;
    const int rr = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(i * 16 + g + 4 * r) * 64 + j * 16 + rr] = acc[i][j][r];
}

// ---------------------------------------------------------------------------
// K1 v3: LDS-shared split-K Gram (aligned fp64 input; the headline path).
//
// Workgroup = 8 waves (2 per SIMD), owns one (group, piece) of the host plan
// (bk_plan.hip): each wave runs one wave-task -- an off-diagonal 64x64
// sub-tile (128 accumulator registers), or the two diagonal sub-tiles of a
// 128-row super-block (upper 16x16 blocks only, 2 x 10 x 8 registers).  The
// group's <= 8 row-blocks are staged ONCE per workgroup through a 4-deep LDS
// ring filled by global_load_lds (16 B per lane, 1 KiB = 16 rows x 64 B per
// instruction, no VGPR staging, 3 k-blocks in flight).  Operands come back by
// ds_read_b128: lane (rr, g) of row-group q reads row 16q+rr, 16-byte granule
// g of the 8-column k-block = columns 2g, 2g+1 = MFMA sub-steps s = 0, 1 (the
// same k permutation for A and B, so the product is X X^T).  Granules are
// XOR-swizzled by (row >> 1) & 3 on the global SOURCE address (glds writes
// lane-linearly) and on the read: conflict-free for ds_read_b128.
// One s_barrier per 8-column k-block (64 MFMAs per SIMD in between).
// ---------------------------------------------------------------------------
// One 16-byte LDS granule in the input type: 2 doubles or 4 floats.  A k-block
// is 8 granules (128 B) per row: 16 fp64 columns or 32 fp32 columns, so the
// LDS image, swizzle and glds shape are the same for both input types.
template <typename T>
struct G3T;
// op / acc: MFMA operand and accumulator types; F32C: the fp32 MFMA, whose
// C/D map is row = 4*(lane>>4) + reg (the f64 one is (lane>>4) + 4*reg)
template <>
struct G3T<double> {
    typedef d2v gran;
    typedef double op;
    typedef d4v acc;
    static constexpr int SUB = 2;   // MFMA sub-steps (k=4 each) per granule
    static constexpr bool F32C = false;
    static __device__ __forceinline__ double at(const d2v &v, int s) { return v[s]; }
    static __device__ __forceinline__ d4v mma(double a, double b, d4v c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
};
template <>
struct G3T<float> {
    typedef f4v gran;
    typedef double op;
    typedef d4v acc;
    static constexpr int SUB = 4;
    static constexpr bool F32C = false;
    // fp32 -> fp64 is exact, and so is every fp32 x fp32 product in fp64
    static __device__ __forceinline__ double at(const f4v &v, int s) { return (double)v[s]; }
    static __device__ __forceinline__ d4v mma(double a, double b, d4v c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
};
// fp32 rows on the fp32 MFMA (bk_set_f32_mode(ctx, BK_F32_MFMA), config E's
// "fp32 MFMA path"): products rounded to fp32 and summed in fp32 within one
// workgroup segment; the segments' partial slabs are summed in fp64 (K1b)
template <>
struct G3T<f32m> {
    typedef f4v gran;
    typedef float op;
    typedef f4v acc;
    static constexpr int SUB = 4;
    static constexpr bool F32C = true;
    static __device__ __forceinline__ float at(const f4v &v, int s) { return v[s]; }
    static __device__ __forceinline__ f4v mma(float a, float b, f4v c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};
// output row of accumulator register r of lane group g in a 16x16 block
template <typename T>
__device__ __forceinline__ constexpr int g3_crow(int g, int r) {
    return G3T<T>::F32C ? 4 * g + r : g + 4 * r;
}

template <typename T>
__device__ __forceinline__ typename G3T<T>::gran g3_frag(const char *lds_blk, int q, int h, int rr,
                                                         int g) {
    const int row = q * 16 + rr;
    return *reinterpret_cast<const typename G3T<T>::gran *>(lds_blk + row * 128 +
                                                            16 * ((4 * h + g) ^ (row & 7)));
}

__device__ __forceinline__ void g3_wait(int vm) {
    switch (vm) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

// the same with the count known at compile time: one instruction, no branch tree
template <int N>
__device__ __forceinline__ void g3_waitc() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void g3_barrier() {
    // every wave's glds for the stage have landed (each waited for its own)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// diagonal sub-tile: upper 16x16 blocks (i <= j) in a flat array of 10
__device__ __forceinline__ constexpr int dix(int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); }

template <int KIND, typename V>
struct G3Acc;
template <typename V>
struct G3Acc<T_OFF, V> {
    V a[4][4];
};
template <typename V>
struct G3Acc<T_PAIR, V> {
    V a[10], b[10];
};
template <typename V>
struct G3Acc<T_DIAG1, V> {
    V a[10];
};

// SKIP: leave block (0,3) to the OFF wave that took it (balanced band quads)
template <typename T, bool SKIP = false>
__device__ __forceinline__ void diag_mma(typename G3T<T>::acc (&acc)[10], const d2v (&a)[4]) {
    typedef typename G3T<T>::op O;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                if (SKIP && i == 0 && j == 3) continue;
                acc[dix(i, j)] = G3T<T>::mma((O)a[i][s], (O)a[j][s], acc[dix(i, j)]);
            }
}
// the ragged-tail OFF product from direct loads (values exact in op)
template <typename T>
__device__ __forceinline__ void off_mma_tail(typename G3T<T>::acc (&acc)[4][4], const d2v (&a)[4],
                                             const d2v (&b)[4]) {
    typedef typename G3T<T>::op O;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = G3T<T>::mma((O)a[i][s], (O)b[j][s], acc[i][j]);
}
// the same over one granule of either input type
template <typename T, bool SKIP = false>
__device__ __forceinline__ void diag_mma_g(typename G3T<T>::acc (&acc)[10],
                                           const typename G3T<T>::gran (&a)[4]) {
#pragma unroll
    for (int s = 0; s < G3T<T>::SUB; ++s) {
        typename G3T<T>::op v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = G3T<T>::at(a[i], s);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                if (SKIP && i == 0 && j == 3) continue;
                acc[dix(i, j)] = G3T<T>::mma(v[i], v[j], acc[dix(i, j)]);
            }
    }
}

template <typename T>
__device__ __forceinline__ void g3_load_rows(d2v (&a)[4], const T *__restrict__ X, int64_t ld,
                                             int n, int b, int64_t c, int64_t d, int rr) {
    // guarded direct loads for the ragged tail (c = first column of this lane)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const T *pr = X + (int64_t)min(b * 64 + q * 16 + rr, n - 1) * ld;
        a[q].x = c < d ? (double)pr[c] : 0.0;
        a[q].y = c + 1 < d ? (double)pr[c + 1] : 0.0;
    }
}

// (wt: write-through stores, a piece handed to the communication stream --
// bk_internal.h piece_done)
template <typename T = double>
__device__ __forceinline__ void store_tile(double *out, const typename G3T<T>::acc (&acc)[4][4],
                                           int rr, int g, bool wt = false) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                st_part(&out[(i * 16 + g3_crow<T>(g, r)) * 64 + j * 16 + rr], (double)acc[i][j][r], wt);
}

template <typename T, bool SKIP = false>
__device__ __forceinline__ void store_diag(double *out, const typename G3T<T>::acc (&acc)[10],
                                           int rr, int g, bool wt = false) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (SKIP && i == 0 && j == 3) continue;  // written by the OFF wave that took it
#pragma unroll
            for (int r = 0; r < 4; ++r)
                st_part(&out[(i * 16 + g3_crow<T>(g, r)) * 64 + j * 16 + rr],
                        j >= i ? (double)acc[dix(i, j)][r] : 0.0, wt);
        }
}

// one MFMA sub-step S (element S of each lane's granule) of an off-diagonal
// tile; XT = 1 / 2: also block (0,3) of the diagonal tile of the A / B row-block
// (operands already in registers: fragments 0 and 3 of that side)
template <typename T, int S, int XT = 0>
__device__ __forceinline__ void off_mma(typename G3T<T>::acc (&acc)[4][4],
                                        const typename G3T<T>::gran (&a)[4],
                                        const typename G3T<T>::gran (&b)[4],
                                        typename G3T<T>::acc &x) {
    typename G3T<T>::op va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        va[i] = G3T<T>::at(a[i], S);
        vb[i] = G3T<T>::at(b[i], S);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = G3T<T>::mma(va[i], vb[j], acc[i][j]);
    if constexpr (XT == 1) x = G3T<T>::mma(va[0], va[3], x);
    if constexpr (XT == 2) x = G3T<T>::mma(vb[0], vb[3], x);
}
// all SUB sub-steps of one granule
template <typename T, int XT = 0>
__device__ __forceinline__ void off_mma_gran(typename G3T<T>::acc (&acc)[4][4],
                                             const typename G3T<T>::gran (&a)[4],
                                             const typename G3T<T>::gran (&b)[4],
                                             typename G3T<T>::acc &x) {
    off_mma<T, 0, XT>(acc, a, b, x);
    off_mma<T, 1, XT>(acc, a, b, x);
    if constexpr (G3T<T>::SUB == 4) {
        off_mma<T, 2, XT>(acc, a, b, x);
        off_mma<T, 3, XT>(acc, a, b, x);
    }
}
// STAG: waves 4-7 (the SIMD partners of waves 0-3) run their OFF tile half a
// k-block behind -- the second 8-column half of block t-1 is issued after the
// barrier of block t, from registers -- so that after every barrier one wave
// of each SIMD has MFMAs ready while its partner waits for its LDS reads.  The
// accumulation order (block by block, column by column) is unchanged, so the
// result is bitwise identical to the unstaggered schedule.
// BK_K1_PROBE (debug builds only): shader cycles spent in the vmcnt wait and
// in the barrier, per wave, reported through the BK_TRACE_FILE timeline
#ifdef BK_K1_PROBE
#define G3_PROBE(v) const long long v = (long long)__builtin_readcyclecounter()
#else
#define G3_PROBE(v) const long long v = 0
#endif
// The glds split (g3_wave): of the 8 NB glds that stage one k-block, waves 0-3
// issue NB + ESPL each and the staggered waves 4-7 NB - ESPL, down to none
// (BK_GLDS_E6 <= 6 for the super pairs' NB = 6, BK_GLDS_E4 <= 4 for the band
// quads' NB = 4).  BK_GLDS_SPREAD = 1: waves 0-3 issue theirs one per
// ceil(MFMAs / glds) MFMAs through the k-block instead of in one burst.
// -DBK_GLDS_E6=2 -DBK_GLDS_E4=2 -DBK_GLDS_SPREAD=0 is the r1-r21 kernel.
#ifndef BK_GLDS_E6
#define BK_GLDS_E6 2
#endif
#ifndef BK_GLDS_E4
#define BK_GLDS_E4 2
#endif
#ifndef BK_GLDS_SPREAD
#define BK_GLDS_SPREAD 1
#endif
#ifndef G3_STAGGER
#define G3_STAGGER 1
#endif
#if defined(BK_K1_NOHIGLDS) && !defined(BK_PROBES)
#error "BK_K1_NOHIGLDS is a timing-only ablation (wrong results): probe builds only"
#endif
// the split follows the stagger: the fp32-MFMA kernel (and a G3_STAGGER = 0
// build) runs unstaggered, so its waves split evenly (the uneven split put the
// fp32 MFMA's band quads' loop at 0.65, even 0.905)
template <typename T, int NB>
__device__ __forceinline__ constexpr int g3_espl() {
    return (G3T<T>::F32C || !G3_STAGGER) ? 0 : NB == 6 ? BK_GLDS_E6 : NB == 4 ? BK_GLDS_E4 : 0;
}
// NB > 0: the group stages exactly NB row-blocks (compile time: a single
// s_waitcnt and straight-line glds); NB = 0: read G.nb at run time.
// XT (balanced band quads, GroupDesc::xt): OFF 1 / 2 = also block (0,3) of the
// A / B row-block's diagonal tile, stored into xout (the PAIR wave's slab);
// PAIR 1 = skip that block in both diagonal tiles
// HI: one of waves 4-7, known at compile time wherever the glds split is
// uneven (g3_espl != 0; g3_dispatch), so that each wave class carries only its
// own glds table
template <typename T, int KIND, int MODE, bool STAG, int NB, int XT = 0, bool HI = STAG>
__device__ __forceinline__ void g3_wave(const T *__restrict__ X, int64_t ld, int n, int nfull,
                                        int64_t d, const GroupDesc &G, const int *wd, char *lds,
                                        int wave, int lane, double *out, long long (&probe)[2],
                                        double *xout = nullptr, bool wt = false) {
    constexpr int XO = KIND == T_OFF ? XT : 0;     // OFF: extra block side
    constexpr bool XP = KIND == T_PAIR && XT != 0;  // PAIR: skip block (0,3)
    typedef typename G3T<T>::gran gran;
    constexpr int EPG = 16 / (int)sizeof(T);  // elements per 16-B granule
    constexpr int BKE = 8 * EPG;               // columns per k-block (16 fp64, 32 fp32)
    const int rr = lane & 15, g = lane >> 4;
    int blk[G3_MAXB];
#pragma unroll
    for (int b = 0; b < G3_MAXB; ++b) blk[b] = G.blk[b];
    const int c = NB > 0 ? NB : G.nb;  // glds per wave per k-block (8 per row-block, 8 waves)
    const int sA = G.task[wave][1], sB = G.task[wave][2];
    const int kst = wd[1], kstr = wd[2], kend = wd[3];
    const int nk = kst < kend ? (kend - 1 - kst) / kstr + 1 : 0;

    // this wave's c (<= 6) glds per k-block: fixed per-lane row pointers and LDS
    // offsets; a stage only adds the k-block's column.  Instruction i of a stage
    // moves rows 8ii..8ii+7 (128 B each) of slot b = i/8; lane L takes row
    // 8ii + L/8, granule (L&7) of the LDS row <- global granule (L&7)^(row&7).
    // ESPL: waves 0-3 issue NB + ESPL of the stage's 8 NB glds and waves 4-7
    // NB - ESPL.  The timeline probe shows waves 0-3 waiting ~2,400-2,600
    // cycles per k-block at the barrier and the staggered waves 4-7 ~100: the
    // latter are the critical path, and each glds costs its wave ~100-185
    // cycles of issue.  Super pairs 6 -> 8 / 4, quads 4 -> 6 / 2: K1 at D
    // 4.07 -> 4.00 ms, the 8-GPU shard and C unchanged (profiles/r01/ab_gldssplit.log);
    // -DBK_GLDS_E6=0 -DBK_GLDS_E4=0 restores the even split.  Which wave issues
    // instruction i never changes the bytes it moves: the LDS image is the same
    // for every split.
    constexpr int ESPL = g3_espl<T, NB>();
    constexpr int CLO = NB + ESPL, CHI = NB - ESPL;
    // this wave's glds per k-block and its table size (uneven split: its class's)
    constexpr int CNT = ESPL != 0 ? (HI ? CHI : CLO) : NB;
    constexpr int GMAX = ESPL != 0 ? (CNT > 0 ? CNT : 1) : G3_MAXB;
    static_assert(ESPL >= 0 && CHI >= 0 && 4 * CLO + 4 * CHI == 8 * NB,
                  "the two wave classes' glds must add up to the stage's 8 NB");
    const T *gsrc[GMAX];
    int gdst[GMAX];
    {
        const int rq = lane >> 3, j = lane & 7;
#pragma unroll
        for (int m = 0; m < GMAX; ++m) {
            // waves 0-3 take instructions 0 .. 4 CLO - 1, waves 4-7 the rest
            int i = wave + 8 * m;
            if constexpr (ESPL != 0) i = HI ? 4 * CLO + (wave - 4) + 4 * m : wave + 4 * m;
            if (i >= 8 * G3_MAXB) i = 0;  // a wave with no glds (CNT = 0): never issued
            const int b = i >> 3, ii = i & 7;
            const int rl = ii * 8 + rq;
#ifdef BK_K1_SAMEROWS  // timing-only ablation: every slot reads row-block 0 (all L2 hits)
            const int grow = min(rl, n - 1);
#else
            const int grow = min(blk[b] * 64 + rl, n - 1);
#endif
            gsrc[m] = X + (int64_t)grow * ld + EPG * (j ^ (rl & 7));
            gdst[m] = b * G3_BLK + ii * 1024;
        }
    }
    auto issue = [&](int64_t kb, int stage) {
#ifdef BK_K1_L2WINDOW  // timing-only ablation: every k-block read from the first W (L2-resident)
        const int64_t col = (kb % BK_K1_L2WINDOW) * BKE;
#else
        const int64_t col = kb * BKE;
#endif
        char *base = lds + stage * G3_STAGE;
#ifndef BK_K1_GLDS_LIMIT  // timing-only ablation: issue at most this many glds per wave
#define BK_K1_GLDS_LIMIT G3_MAXB
#endif
        if constexpr (ESPL != 0) {
#pragma unroll
            for (int m = 0; m < CNT; ++m)
                __builtin_amdgcn_global_load_lds((const void *)(gsrc[m] + col),
                                                 (void *)(base + gdst[m]), 16, 0, 0);
            return;
        }
#pragma unroll
        for (int m = 0; m < (NB > 0 ? NB : G3_MAXB); ++m)
            if ((NB > 0 || m < c) && m < BK_K1_GLDS_LIMIT)
                __builtin_amdgcn_global_load_lds((const void *)(gsrc[m] + col),
                                                 (void *)(base + gdst[m]), 16, 0, 0);
    };

    typedef typename G3T<T>::acc AV;
    G3Acc<KIND == T_NONE ? T_DIAG1 : KIND, AV> acc;
    if constexpr (KIND == T_OFF) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc.a[i][j] = AV{0, 0, 0, 0};
    } else if constexpr (KIND == T_PAIR) {
#pragma unroll
        for (int i = 0; i < 10; ++i) acc.a[i] = acc.b[i] = AV{0, 0, 0, 0};
    } else if constexpr (KIND == T_DIAG1) {
#pragma unroll
        for (int i = 0; i < 10; ++i) acc.a[i] = AV{0, 0, 0, 0};
    }
    AV xacc = AV{0, 0, 0, 0};  // XO: the extra diagonal block
    gran ha[4], hb[4];  // STAG: the held second granule of the previous k-block
#pragma unroll
    for (int q = 0; q < 4; ++q) ha[q] = hb[q] = gran{};

#pragma unroll
    for (int s = 0; s < G3_STAGES - 1; ++s)
        if (s < nk && MODE != 2) issue(kst + (int64_t)s * kstr, s);
#ifdef BK_K1_NOHIGLDS  // timing-only ablation: waves 4-7 stage nothing after the prologue
    constexpr bool NOHI = HI && ESPL != 0;
#else
    constexpr bool NOHI = false;
#endif
    // every glds of stage t + 2 is issued after barrier t and before the wait of
    // k-block t + 1, which leaves exactly that stage's CNT outstanding
    constexpr int WCNT = NOHI ? 0 : CNT;
    // SPR: waves 0-3 spread their glds through the k-block's MFMAs.  That
    // needs the k-block in one basic block, so the k-blocks that still stage
    // (STEADY: t + 2 < nk, no run-time "more") are peeled from the last two.
    // fp64 rows only: on widened fp32 rows the spread order keeps the converted
    // operands alive across the glds and spills (664 B of scratch per lane)
    constexpr bool SPR = BK_GLDS_SPREAD && ESPL != 0 && MODE == 0 && std::is_same<T, double>::value;
    int buf = 0, t = 0;
    if constexpr (SPR) {
        for (; t + G3_STAGES - 1 < nk; ++t) {
            constexpr bool STEADY = true;
#include "bk_gram_kblock.inc"
        }
    }
    for (; t < nk; ++t) {
        constexpr bool STEADY = false;
#include "bk_gram_kblock.inc"
    }
    if constexpr (KIND == T_OFF && STAG && MODE != 1)
        if (nk > 0) off_mma_gran<T, XO>(acc.a, ha, hb, xacc);
    if constexpr (KIND != T_NONE) {
        // ragged tail columns [nfull*BKE, d): one workgroup per group, direct loads
        const int64_t c0 = (int64_t)nfull * BKE;
        if (wd[4] && c0 < d) {
#pragma unroll
            for (int h = 0; h < BKE / 8; ++h) {
                const int64_t cc = c0 + 8 * h + 2 * g;
                d2v a[4], b[4];
                g3_load_rows<T>(a, X, ld, n, blk[sA], cc, d, rr);
                g3_load_rows<T>(b, X, ld, n, blk[sB], cc, d, rr);
                if constexpr (KIND == T_OFF) {
                    typedef typename G3T<T>::op O;
                    off_mma_tail<T>(acc.a, a, b);
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        if constexpr (XO == 1) xacc = G3T<T>::mma((O)a[0][s2], (O)a[3][s2], xacc);
                        if constexpr (XO == 2) xacc = G3T<T>::mma((O)b[0][s2], (O)b[3][s2], xacc);
                    }
                } else if constexpr (KIND == T_PAIR) {
                    diag_mma<T, XP>(acc.a, a);
                    diag_mma<T, XP>(acc.b, b);
                } else {
                    diag_mma<T>(acc.a, a);
                }
            }
        }
        if constexpr (KIND == T_OFF) {
            store_tile<T>(out, acc.a, rr, g, wt);
            if constexpr (XO != 0) {  // block (0,3) of the PAIR wave's diagonal tile
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    st_part(&xout[g3_crow<T>(g, r) * 64 + 48 + rr], (double)xacc[r], wt);
            }
        } else if constexpr (KIND == T_PAIR) {
            store_diag<T, XP>(out, acc.a, rr, g, wt);
            store_diag<T, XP>(out + 4096, acc.b, rr, g, wt);
        } else {
            store_diag<T>(out, acc.a, rr, g, wt);
        }
    }
}

template <typename T, int MODE, int NB>
__device__ __forceinline__ void g3_dispatch(const T *__restrict__ X, int64_t ld, int n,
                                            int nfull, int64_t d, const GroupDesc &G,
                                            const int *wd, char *lds, int wave, int lane,
                                            double *out, long long (&probe)[2], bool wt) {
    // the balanced quads always stage 4 row-blocks: only NB = 4 (and the
    // run-time NB = 0 of the ablation modes) carries the XT variants
    const int xt = (NB == 4 || NB == 0) ? G.xt[wave] : 0;
    // an uneven glds split: the wave's class (0-3 / 4-7) is a template argument.
    // It follows the stagger, so an OFF wave's class is its STAG
    constexpr bool SPLIT = g3_espl<T, NB>() != 0;
    double *xout = out - (int64_t)wave * 2 * 4096 + (int64_t)G.xslot[wave] * 4096;
    switch (G.task[wave][0]) {
    case T_OFF:
        // the stagger covers the fp64 MFMA's 64-cycle issue; on the fp32 MFMA
        // (32 cycles) it costs more than it hides: E's loop efficiency 0.776
        // staggered, 0.845 not (tools/trace_gram.py)
#ifndef BK_F32_STAGGER  // probe knob: 1 staggers the fp32-MFMA kernel too
#define BK_F32_STAGGER 0
#endif
        if (wave >= 4 && G3_STAGGER && (!G3T<T>::F32C || BK_F32_STAGGER)) {
            if (xt == 1)
                g3_wave<T, T_OFF, MODE, true, NB, (NB == 4 || NB == 0) ? 1 : 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, xout, wt);
            else if (xt == 2)
                g3_wave<T, T_OFF, MODE, true, NB, (NB == 4 || NB == 0) ? 2 : 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, xout, wt);
            else
                g3_wave<T, T_OFF, MODE, true, NB>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        } else {
            if (xt == 1)
                g3_wave<T, T_OFF, MODE, false, NB, (NB == 4 || NB == 0) ? 1 : 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, xout, wt);
            else if (xt == 2)
                g3_wave<T, T_OFF, MODE, false, NB, (NB == 4 || NB == 0) ? 2 : 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, xout, wt);
            else
                g3_wave<T, T_OFF, MODE, false, NB>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        }
        break;
    case T_PAIR:
        if (SPLIT && wave >= 4) {
            if (xt)
                g3_wave<T, T_PAIR, MODE, false, NB, (NB == 4 || NB == 0) ? 1 : 0, SPLIT>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
            else
                g3_wave<T, T_PAIR, MODE, false, NB, 0, SPLIT>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        } else {
            if (xt)
                g3_wave<T, T_PAIR, MODE, false, NB, (NB == 4 || NB == 0) ? 1 : 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
            else
                g3_wave<T, T_PAIR, MODE, false, NB>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        }
        break;
    case T_DIAG1:
        if (SPLIT && wave >= 4)
            g3_wave<T, T_DIAG1, MODE, false, NB, 0, SPLIT>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        else
            g3_wave<T, T_DIAG1, MODE, false, NB>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        break;
    default:
        if (SPLIT && wave >= 4)
            g3_wave<T, T_NONE, MODE, false, NB, 0, SPLIT>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        else
            g3_wave<T, T_NONE, MODE, false, NB>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, nullptr, wt);
        break;
    }
}
template <int MODE, typename T = double>
__global__ __launch_bounds__(512, 2) void k_gram3(const T *__restrict__ X, int64_t ld, int n,
                                                  int nfull, int64_t d,
                                                  const GroupDesc *__restrict__ groups,
                                                  const int *__restrict__ segtab,
                                                  const int *__restrict__ wgtab,
                                                  double *__restrict__ part,
                                                  long long *__restrict__ trace, PieceMarks pm) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // debug timeline (BK_TRACE_FILE): per workgroup 100 MHz start/end, shader
    // clock start/end, HW_ID, XCC_ID
    long long t_rt0 = 0, t_mt0 = 0;
    if (trace && threadIdx.x == 0) {
        t_rt0 = (long long)__builtin_amdgcn_s_memrealtime();
        t_mt0 = (long long)__builtin_amdgcn_s_memtime();
    }
    long long probe[2] = {0, 0};
    const bool wt = piece_handed(pm) && !pm.nowt;  // this workgroup's slabs go to the communication stream
    const int v0 = segtab[2 * blockIdx.x], nseg = segtab[2 * blockIdx.x + 1];
    long long ideal = 0;  // sum of nk * cost over the segments (trace only)
    for (int sg = 0; sg < nseg; ++sg) {
        const int v = v0 + sg;
        const int *wd = wgtab + 5 * v;
        const GroupDesc &G = groups[wd[0]];
        double *out = part + ((int64_t)v * 16 + wave * 2) * 4096;
        if (sg > 0) __syncthreads();  // the previous segment's waves are done with the LDS ring
        if constexpr (MODE == 0) {
            switch (G.nb) {
            case 1: g3_dispatch<T, MODE, 1>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            case 2: g3_dispatch<T, MODE, 2>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            case 3: g3_dispatch<T, MODE, 3>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            case 4: g3_dispatch<T, MODE, 4>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            case 5: g3_dispatch<T, MODE, 5>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            default: g3_dispatch<T, MODE, 6>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt); break;
            }
        } else {
            g3_dispatch<T, MODE, 0>(X, ld, n, nfull, d, G, wd, lds, wave, lane, out, probe, wt);
        }
        if (trace) ideal += (long long)(wd[1] < wd[3] ? (wd[3] - 1 - wd[1]) / wd[2] + 1 : 0) * G.cost;
    }
    piece_done(pm);
    if (trace) {
#ifdef BK_K1_PROBE
        if (lane == 0) {
            trace[24 * blockIdx.x + 8 + wave] = probe[0];
            trace[24 * blockIdx.x + 16 + wave] = probe[1];
        }
#endif
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            long long *tr = trace + 24 * blockIdx.x;
            tr[0] = t_rt0;
            tr[1] = (long long)__builtin_amdgcn_s_memrealtime();
            tr[2] = t_mt0;
            tr[3] = (long long)__builtin_amdgcn_s_memtime();
            tr[4] = hw;
            tr[5] = xcc;
            // first segment's group and cost; k-blocks scaled so nk * cost = the ideal
            const int g0 = nseg > 0 ? wgtab[5 * v0] : 0;
            const int c0 = groups[g0].cost > 0 ? groups[g0].cost : 1;
            tr[6] = g0 | ((long long)c0 << 32);
            tr[7] = (ideal + c0 / 2) / c0;
        }
    }
}

// K1b v3: U[u] = sum over the owning group's workgroups (fixed order) of its slab
// block = 32 elements of one sub-tile x 8 interleaved sub-lists of its
// workgroups' slabs (sub-list q sums slabs q, q+8, q+16, ... in order), then
// the 8 sub-sums in order: a fixed order (deterministic), with 8x the loads in
// flight of one serial chain -- small-n plans have ~256 slabs per sub-tile
__global__ __launch_bounds__(256) void k_reduce3(const double *__restrict__ part,
                                                 const int *__restrict__ red,
                                                 const int *__restrict__ wglist,
                                                 double *__restrict__ U, int64_t usz,
                                                 double dcols, double dcols32, int u0, int rec) {
    // the packed upper's two trailing elements: the Gram's column count, and
    // how many of those columns were accumulated at fp32 unit roundoff (the
    // fp32 MFMA); both are summed with the tiles by every exchange, so after
    // one they are totals (K3b's margin: the total d, and u_G = 2^-24 as soon
    // as any shard ran on the fp32 MFMA)
    // (u0 / rec: one piece of the packed upper -- sub-tiles from u0 on, the
    // record only with the last piece -- when the exchange overlaps the Gram)
    if (rec && blockIdx.x == 0 && threadIdx.x == 0) {
        U[usz] = dcols;
        U[usz + 1] = dcols32;
        U[usz + 2] = 0.0;  // no int8-sliced columns
        U[usz + 3] = 0.0;
    }
    // 64 elements per block, 2 per lane (16-B loads), 8 slabs in flight per
    // sub-list; the same order of adds as one element per lane (bitwise the same U)
    __shared__ d2v sub[8][32];
    const int u = u0 + (blockIdx.x >> 6), el = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int e = (blockIdx.x & 63) * 64 + el * 2;
    const int off = red[3 * u], np = red[3 * u + 1], slot = red[3 * u + 2];
    const int *wl = wglist + off;
    d2v acc = {0.0, 0.0};
    int s = q;
    for (; s + 56 < np; s += 64) {
        d2v v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = *reinterpret_cast<const d2v *>(part + ((int64_t)wl[s + 8 * k] * 16 + slot) * 4096 + e);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc.x += v[k].x;
            acc.y += v[k].y;
        }
    }
    for (; s < np; s += 8) {
        const d2v v = *reinterpret_cast<const d2v *>(part + ((int64_t)wl[s] * 16 + slot) * 4096 + e);
        acc.x += v.x;
        acc.y += v.y;
    }
    sub[q][el] = acc;
    __syncthreads();
    if (q == 0) {
        d2v t = sub[0][el];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            t.x += sub[k][el].x;
            t.y += sub[k][el].y;
        }
        *reinterpret_cast<d2v *>(U + (int64_t)u * 4096 + e) = t;
    }
}

// ---------------------------------------------------------------------------
// K1b: packed upper U[u][64][64] = sum_{s=0..S-1} part[s*ntile+u] (fixed order)
// grid: ntile*16 blocks of 256 threads (4 rows x 64 cols each)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reduce(const double *__restrict__ part, int ntile, int S,
                                                double *__restrict__ U, double dcols) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // as k_reduce3 (v1 never runs the fp32 MFMA)
        U[(int64_t)ntile * 4096] = dcols;
        U[(int64_t)ntile * 4096 + 1] = 0.0;
        U[(int64_t)ntile * 4096 + 2] = 0.0;
        U[(int64_t)ntile * 4096 + 3] = 0.0;
    }
    const int u = blockIdx.x >> 4, chunk = blockIdx.x & 15;
    const int e = chunk * 256 + threadIdx.x;
    const double *p = part + (int64_t)u * 4096 + e;
    const int64_t stride = (int64_t)ntile * 4096;
    double acc = 0.0;
    int s = 0;
    for (; s + 4 <= S; s += 4) {
        const double v0 = p[(s + 0) * stride], v1 = p[(s + 1) * stride];
        const double v2 = p[(s + 2) * stride], v3 = p[(s + 3) * stride];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
    }
    for (; s < S; ++s) acc += p[s * stride];
    U[(int64_t)u * 4096 + e] = acc;
}

// Fixed-order sum of R packed partials (deterministic multi-GPU mode):
// U[e] = sum_{r=0..R-1} Ug[r*stride + e]
__global__ __launch_bounds__(256) void k_sum_ranks(const double *__restrict__ Ug, int R,
                                                   int64_t stride, double *__restrict__ U) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= stride) return;
    double acc = 0.0;
    for (int r = 0; r < R; ++r) acc += Ug[(int64_t)r * stride + e];
    U[e] = acc;
}

// ===========================================================================
// launchers
// ===========================================================================

static constexpr int GRAM_P = 4;

hipError_t launch_gram(const void *X, int dtype, int64_t ld, int n, int64_t d, const Plan &pl,
                       double *part, hipStream_t st) {
    const dim3 grid((unsigned)pl.nwg), block(256);
    with_row_type(dtype, rows_pair_aligned(X, dtype, ld), [&](auto t, auto vec) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_gram<T, decltype(vec)::value, GRAM_P>), grid, block, 0, st,
                           (const T *)X, ld, n, d, pl.T, pl.ntile, pl.S, pl.kc, pl.nwg, part);
    });
    return hipGetLastError();
}

hipError_t launch_reduce(const double *part, const Plan &pl, double *U, hipStream_t st) {
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)pl.ntile * 16), dim3(256), 0, st, part, pl.ntile,
                       pl.S, U, (double)pl.d);
    return hipGetLastError();
}

// U[e] += P[e]: the host entries' running sum of column-chunk Gram partials
// (chunk order, so deterministic)
__global__ __launch_bounds__(256) void k_add_upper(double *__restrict__ U,
                                                   const double *__restrict__ P, int64_t count) {
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (e + 1 < count) {
        d2v u = *reinterpret_cast<const d2v *>(U + e), p = *reinterpret_cast<const d2v *>(P + e);
        *reinterpret_cast<d2v *>(U + e) = u + p;
    } else if (e < count) {
        U[e] += P[e];
    }
}

hipError_t launch_add_upper(double *U, const double *P, int64_t count, hipStream_t st) {
    hipLaunchKernelGGL(k_add_upper, dim3((unsigned)((count + 511) / 512)), dim3(256), 0, st, U, P,
                       count);
    return hipGetLastError();
}

hipError_t launch_sum_ranks(const double *Ug, int R, int64_t stride, double *U, hipStream_t st) {
    hipLaunchKernelGGL(k_sum_ranks, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, st, Ug, R,
                       stride, U);
    return hipGetLastError();
}

hipError_t launch_gram3(const void *X, int dtype, int64_t ld, int n, int64_t d, const Plan3 &pl0,
                        double *part, hipStream_t st, int mode, long long *trace, bool f32_mfma,
                        const int *seg, int nwg, const PieceMarks &pm) {
    // mode != 0: timing-only ablations (1: no MFMA, 2: no global loads) -- wrong
    // results, so they exist only in probe builds (-DBK_PROBES); the product ignores mode
    (void)mode;
    // seg / nwg: one piece's launch table (the exchange overlapping the Gram):
    // the same segments and slabs, a subset of the launched workgroups
    Plan3 pl = pl0;
    if (seg) {
        pl.d_seg = const_cast<int *>(seg);
        pl.nwg = nwg;
    }
    if (pl.nwg < 1) return hipSuccess;
    const dim3 grid((unsigned)pl.nwg), block(512);
    if (dtype != 0 && f32_mfma)  // fp32 input on the fp32 MFMA
        hipLaunchKernelGGL((k_gram3<0, f32m>), grid, block, G3_LDS, st, (const f32m *)X, ld, n,
                           pl.nfull, d, pl.d_groups, pl.d_seg, pl.d_wg, part, trace, pm);
    else if (dtype != 0)  // fp32 input, exact (widened onto the fp64 MFMA): production mode only
        hipLaunchKernelGGL((k_gram3<0, float>), grid, block, G3_LDS, st, (const float *)X, ld, n,
                           pl.nfull, d, pl.d_groups, pl.d_seg, pl.d_wg, part, trace, pm);
#ifdef BK_PROBES
    else if (mode == 1)
        hipLaunchKernelGGL(k_gram3<1>, grid, block, G3_LDS, st, (const double *)X, ld, n, pl.nfull,
                           d, pl.d_groups, pl.d_seg, pl.d_wg, part, trace, pm);
    else if (mode == 2)
        hipLaunchKernelGGL(k_gram3<2>, grid, block, G3_LDS, st, (const double *)X, ld, n, pl.nfull,
                           d, pl.d_groups, pl.d_seg, pl.d_wg, part, trace, pm);
#endif
    else
        hipLaunchKernelGGL(k_gram3<0>, grid, block, G3_LDS, st, (const double *)X, ld, n, pl.nfull,
                           d, pl.d_groups, pl.d_seg, pl.d_wg, part, trace, pm);
    return hipGetLastError();
}

hipError_t launch_reduce3(const double *part, const Plan3 &pl, double *U, hipStream_t st,
                          bool f32_mfma, int u0, int u1, bool rec) {
    const int64_t usz = (int64_t)pl.ntile * 4096;
    const double d32 = f32_mfma ? (double)pl.d : 0.0;
    if (u1 < 0) u1 = pl.ntile;
    if (u1 <= u0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce3, dim3((unsigned)(u1 - u0) * 64), dim3(256), 0, st, part, pl.d_red,
                       pl.d_wglist, U, usz, (double)pl.d, d32, u0, rec ? 1 : 0);
    return hipGetLastError();
}

hipError_t configure_gram_kernels() {
    for (const void *k : {(const void *)k_gram3<0>, (const void *)k_gram3<0, float>,
                          (const void *)k_gram3<0, f32m>,
#ifdef BK_PROBES  // the timing-only K1 ablations (BK_GRAM_MODE)
                          (const void *)k_gram3<1>, (const void *)k_gram3<2>,
#endif
         }) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, G3_LDS);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace bk
