// bk_scores.hip -- the scoring and selection stages of the Multi-Krum engine,
// CDNA4 (gfx950).
//
// The middle steps of one Multi-Krum call (DESIGN.md "Kernels"; K1 is in
// bk_gram.hip, K4 in bk_mean.hip):
//   K2  k_scores2   per row: D_ij = (G_ii + G_jj) - 2 G_ij read straight from the
//                   packed upper tiles (no n x n expansion; for large n from
//                   k_transpose's transposed tiles), bitonic sort in registers
//                   (NaN last), sum of ranks 1..k      (logistic_validator.py:62-63)
//   K3  k_rank      rank of each score (ties -> lower index, NaN last), mask
//   K3b k_compact   mask -> ascending selected indices (argpartition set, :45)
// and k_split_unpack, which gathers the scores a sharded call scored by ranks.
//
// Built with -ffp-contract=off: every add/mul rounds exactly as the numpy
// reference evaluates it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "bk_device.h"
#include "bk_internal.h"

namespace bk {

// ---------------------------------------------------------------------------
// K2: score[i] = sum of ranks 1..k of sort(D[i])   (logistic_validator.py:62-63)
// One workgroup per row.  "v1" below is the first K2, retired since (DESIGN.md
// §4): the row in LDS as order-preserving u64 keys (dkey), an LDS bitonic
// sort, and the sum by 256 threads (1024 above 2048 keys).  Its key order and
// its summation shape still define the bits of every score.
// ---------------------------------------------------------------------------
// K2 v2: the same scores, bitwise, with the row's keys in REGISTERS.  Thread
// t holds keys t*KPT .. t*KPT+KPT-1 (blocked).  Bitonic stages with a stride
// below KPT are compare-exchanges inside a thread; strides up to the wave's
// span (64 KPT keys) exchange across lanes -- DPP quad permutes for lane xor
// 1 / 2, ds_swizzle (bit-mask mode, no LDS banks) for 4 / 8 / 16, ds_bpermute
// for 32 -- with no barriers; only strides beyond a wave go through LDS.
// Keys are the distances as fp64 (-0 -> +0), ordered by v_min/v_max_f64 (two
// instructions per compare-exchange); a row holding a NaN (rare: NaN / Inf
// updates) is sorted as v1's order-preserving u64 keys instead (NaN last).
// The sorted row is written to LDS once and summed in v1's exact shape: v1's
// NT_SUM threads (256, or 1024 above 2048 keys), each summing ranks 1+t,
// 1+t+NT_SUM, ..., the wave butterfly, then the waves in order -- emulated
// with H = NT_SUM / NT accumulators per thread.  Any correct sort of the same
// keys gives the same array, so the scores are bitwise v1's.
// Row loads: from the packed upper tiles (u_at), or -- for large n, after
// k_transpose -- from Ut (the off-diagonal tiles transposed) and a contiguous
// diagonal, so a row is read in 512-B runs instead of 8-B strided elements.
// bitonic sort of N = NT * KPT keys, blocked (thread t holds keys t KPT ..),
// in the all-ascending form: each merge of size s opens with the mirror stage
// (partner e ^ (s - 1)) and continues with xor stages (e ^ s/4, ..., e ^ 1);
// the lower index of every pair takes the minimum, so no stage needs a
// direction.  The sorted keys end in keys_lds.
template <typename K, int NT, int KPT>
__device__ __forceinline__ void k2_sort(K (&v)[KPT], K *keys_lds, int N, int tid) {
    constexpr int LK = KPT == 1 ? 0 : KPT == 2 ? 1 : KPT == 4 ? 2 : KPT == 8 ? 3 : 4;
    constexpr int WSPAN = 64 * KPT;  // keys per wave
    const int lane = tid & 63, e0 = tid * KPT;
    for (int size = 2; size <= N; size <<= 1) {
        // (1) the mirror stage
        if (size <= KPT) {
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const int p = q ^ (size - 1);
                if (q < p && ((q ^ p) & (size >> 1))) k2_cas(v[q], v[p]);
            }
        } else if (size <= WSPAN) {
            const int m = (size - 1) >> LK;
            k2_lane_dispatch<K, KPT, KPT - 1>(v, m, (lane & ((size >> 1) >> LK)) == 0);
        } else {
            __syncthreads();  // earlier readers of keys_lds are done
#pragma unroll
            for (int q = 0; q < KPT; ++q) keys_lds[e0 + q] = v[q];
            __syncthreads();
            const int half = size >> 1;
            for (int p = tid; p < (N >> 1); p += NT) {
                const int lo = (p / half) * size + (p & (half - 1));
                const int hi = lo ^ (size - 1);
                K a = keys_lds[lo], b = keys_lds[hi];
                k2_cas(a, b);
                keys_lds[lo] = a;
                keys_lds[hi] = b;
            }
            __syncthreads();
            // (2a) xor stages beyond the wave, still in LDS
            int stride = size >> 2;
            for (; stride >= WSPAN; stride >>= 1) {
                for (int p = tid; p < (N >> 1); p += NT) {
                    const int lo = 2 * p - (p & (stride - 1));
                    const int hi = lo + stride;
                    K a = keys_lds[lo], b = keys_lds[hi];
                    k2_cas(a, b);
                    keys_lds[lo] = a;
                    keys_lds[hi] = b;
                }
                __syncthreads();
            }
#pragma unroll
            for (int q = 0; q < KPT; ++q) v[q] = keys_lds[e0 + q];
        }
        // (2b) xor stages across lanes, then (2c) inside the thread
        for (int stride = min(size >> 2, WSPAN >> 1); stride >= KPT; stride >>= 1) {
            const int m = stride >> LK;
            k2_lane_dispatch<K, KPT, 0>(v, m, (lane & m) == 0);
        }
#pragma unroll
        for (int st = KPT / 2; st >= 1; st >>= 1) {
            if (st > (size >> 2)) continue;
#pragma unroll
            for (int q = 0; q < KPT; ++q)
                if ((q & st) == 0) k2_cas(v[q], v[q + st]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KPT; ++q) keys_lds[e0 + q] = v[q];
    __syncthreads();
}

// K2 v3 sort, 16 keys per thread (N >= 4096): every compare-exchange inside a
// thread.  A stage on index bit b is register-local when b is one of the 4
// bits the current layout keeps in the register index; layout L_j keeps bits
// j .. j+3 there (thread t, register q hold key e = (t mod 2^j) | q 2^j |
// (t >> j) 2^(j+4)), and a merge of 2^B keys walks its bits B-1 .. 0 in
// chunks of 4, moving the keys to L_(hi-3) .. L_0 through LDS before each
// chunk (3 moves per merge at N = 4096, 20 in all) instead of lane exchanges
// (v2: 33 DPP / swizzle / bpermute stages of ~6 instructions per key).  The
// merges use the classic alternating directions, folded into the keys:
// before merge B the keys of blocks with bit B set are negated (order
// reversed: -x for fp64, ~x for the u64 keys), so every stage keeps the
// minimum at the lower index and the sequence entering each merge is bitonic;
// at B = log2 N nothing is negated.  LDS words are padded by one per 16 keys
// (word e + e/16), which keeps every layout's 16-lane write groups and 32-lane
// read groups on distinct banks.  Any correct sort gives the same array.
__device__ __forceinline__ int k2_pad(int e) { return e + (e >> 4); }
template <int J>
__device__ __forceinline__ int k2_lbase(int t) {
    const int e = (t & ((1 << J) - 1)) | ((t >> J) << (J + 4));
    return e + (e >> 4);
}
template <int J>
__device__ __forceinline__ constexpr int k2_loff(int q) {  // padded word of (t, q) - of (t, 0)
    if constexpr (J >= 4)
        return (q << J) + (q << (J - 4));
    else
        return (q << J) + (q >> (4 - J));
}
template <typename K, int J>
__device__ __forceinline__ void k2_put(const K (&v)[16], K *lds, int t) {
    K *p = lds + k2_lbase<J>(t);
#pragma unroll
    for (int q = 0; q < 16; ++q) p[k2_loff<J>(q)] = v[q];
}
template <typename K, int J>
__device__ __forceinline__ void k2_get(K (&v)[16], const K *lds, int t) {
    const K *p = lds + k2_lbase<J>(t);
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = p[k2_loff<J>(q)];
}
// the ordering point of a move: a workgroup barrier, or -- when every key
// stays inside its wave -- only a compiler fence (a wave's LDS operations
// execute in order, so its reads see its own lanes' writes)
__device__ __forceinline__ void k2_sync(bool local) {
    if (local) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}
// L_from -> L_to.  Thread bits 6.. (the wave index) are key bits 10.. in every
// layout L_j with j <= 6, so a move between two such layouts keeps each key in
// its wave, in the wave's own LDS words: no workgroup barrier (16 of the 20
// moves at N = 4096)
template <typename K>
__device__ __forceinline__ void k2_move(K (&v)[16], K *lds, int t, int from, int to) {
    const bool local = from <= 6 && to <= 6;
    k2_sync(local);  // earlier readers of these words are done
    switch (from) {
    case 0: k2_put<K, 0>(v, lds, t); break;
    case 1: k2_put<K, 1>(v, lds, t); break;
    case 2: k2_put<K, 2>(v, lds, t); break;
    case 3: k2_put<K, 3>(v, lds, t); break;
    case 4: k2_put<K, 4>(v, lds, t); break;
    case 5: k2_put<K, 5>(v, lds, t); break;
    case 6: k2_put<K, 6>(v, lds, t); break;
    case 7: k2_put<K, 7>(v, lds, t); break;
    case 8: k2_put<K, 8>(v, lds, t); break;
    case 9: k2_put<K, 9>(v, lds, t); break;
    default: k2_put<K, 10>(v, lds, t); break;
    }
    k2_sync(local);
    switch (to) {
    case 0: k2_get<K, 0>(v, lds, t); break;
    case 1: k2_get<K, 1>(v, lds, t); break;
    case 2: k2_get<K, 2>(v, lds, t); break;
    case 3: k2_get<K, 3>(v, lds, t); break;
    case 4: k2_get<K, 4>(v, lds, t); break;
    case 5: k2_get<K, 5>(v, lds, t); break;
    case 6: k2_get<K, 6>(v, lds, t); break;
    case 7: k2_get<K, 7>(v, lds, t); break;
    case 8: k2_get<K, 8>(v, lds, t); break;
    case 9: k2_get<K, 9>(v, lds, t); break;
    default: k2_get<K, 10>(v, lds, t); break;
    }
}
// an ascending stage on register bit R (pairs q, q + 2^R)
template <typename K, int R>
__device__ __forceinline__ void k2_rstage(K (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (!(q & (1 << R))) k2_cas(v[q], v[q | (1 << R)]);
}
template <typename K>
__device__ __forceinline__ void k2_rstages(K (&v)[16], int top) {  // register bits top .. 0
    switch (top) {
    case 3: k2_rstage<K, 3>(v); [[fallthrough]];
    case 2: k2_rstage<K, 2>(v); [[fallthrough]];
    case 1: k2_rstage<K, 1>(v); [[fallthrough]];
    default: k2_rstage<K, 0>(v);
    }
}
template <typename K>
__device__ __forceinline__ void k2_negate(K (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = K2Ord<K>::neg(v[q]);
}
// v: thread t's keys t*16 .. t*16+15 (L_0); on return the whole row sorted
// ascending sits in lds at the padded words k2_pad(e)
template <typename K>
__device__ __forceinline__ void k2_sort16(K (&v)[16], K *lds, int N, int tid) {
    if (tid & 1) k2_negate(v);  // blocks of 16 with bit 4 set sort descending
    // merges of 2 .. 16 keys inside the thread (all-ascending mirror form)
#pragma unroll
    for (int size = 2; size <= 16; size <<= 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int p = q ^ (size - 1);
            if (q < p && ((q ^ p) & (size >> 1))) k2_cas(v[q], v[p]);
        }
#pragma unroll
        for (int st = size >> 2; st >= 1; st >>= 1)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((q & st) == 0) k2_cas(v[q], v[q + st]);
    }
    for (int B = 5; (1 << B) <= N; ++B) {
        if (((tid >> (B - 4)) ^ (tid >> (B - 5))) & 1) k2_negate(v);  // direction of merge B
        int cur = 0;
        for (int hi = B - 1; hi >= 0;) {
            const int j = hi > 3 ? hi - 3 : 0;
            k2_move(v, lds, tid, cur, j);
            cur = j;
            k2_rstages(v, hi - j);
            hi = j - 1;
        }
    }
    __syncthreads();
    k2_put<K, 0>(v, lds, tid);
    __syncthreads();
}

// v1's summation shape over the sorted keys (virtual thread t' = tid + NT h)
// ranks >= nfin hold NaN (v1's keys sort NaN after +inf; v2/v3 sort the NaN
// distances as +inf and put the NaN back here, at the same ranks)
template <typename K, int NT, int NT_SUM, bool PAD = false>
__device__ __forceinline__ double k2_sum(const K *keys_lds, int64_t k, int tid, double *red,
                                         int64_t nfin = INT64_MAX) {
    constexpr int H = NT_SUM / NT;
    const int lane = tid & 63;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        double acc = 0.0;
        for (int64_t r = 1 + tid + NT * h; r <= k; r += NT_SUM)
            acc += r < nfin ? K2Ord<K>::val(keys_lds[PAD ? k2_pad((int)r) : r]) : __builtin_nan("");
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) red[(tid >> 6) + (NT / 64) * h] = acc;
    }
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < NT_SUM / 64; ++w) sum += red[w];
    return sum;
}

// row i of G, element e: packed upper tiles, or (TR) Ut + contiguous diagonal
template <bool TR>
__device__ __forceinline__ double k2_g(const double *__restrict__ U, const double *__restrict__ Ut,
                                       int T_, int i, int e) {
    if constexpr (!TR) {
        return u_at(U, T_, i, e);
    } else {
        const int br = i >> 6, bc = e >> 6, ir = i & 63, ic = e & 63;
        if (br < bc || (br == bc && ir <= ic)) return U[upper_tile(T_, br, bc) + ir * 64 + ic];
        if (br == bc) return U[upper_tile(T_, br, br) + ic * 64 + ir];
        return Ut[upper_tile(T_, bc, br) + ir * 64 + ic];  // (Ut tile) = (U tile)^T
    }
}

// MODE (timing-only ablations, tools/k2_modes.py): 1 = loads and keys, no
// sort; 2 = sort of synthetic keys, no loads
template <int NT, int KPT, int NT_SUM, bool TR, int MODE = 0>
__global__ __launch_bounds__(NT) void k_scores2(const double *__restrict__ U,
                                                const double *__restrict__ Ut,
                                                const double *__restrict__ dg_in, int T_, int n,
                                                int N, int64_t k, double *__restrict__ scores,
                                                double *__restrict__ diag, int r0) {
    static_assert(NT_SUM % NT == 0 && NT % 64 == 0, "summation shape");
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // N
    __shared__ double red[NT_SUM / 64];
    // row i: workgroup b scores row r0 + b (a rank's share of the rows when the
    // scoring is split over the ranks of a sharded call; r0 = 0 otherwise)
    const int i = r0 + (int)blockIdx.x, tid = threadIdx.x;
    const double di = TR ? dg_in[i] : u_at(U, T_, i, i);
    if (tid == 0) diag[i] = di;
    // distances, element e = tid + NT q (consecutive lanes, consecutive
    // columns: coalesced row reads), through LDS into the blocked layout.  A
    // NaN distance sorts as +inf and is counted: v1's order puts the row's
    // NaNs right after every +inf and before the padding, i.e. at ranks
    // n - nan .. n - 1, and k2_sum adds NaN there -- the same scores, bitwise,
    // without a second (u64-key) sort in the kernel (its registers held K2 at
    // 3 waves per SIMD)
    constexpr bool V3 = KPT == 16;  // the register-local sort (k2_sort16)
    __shared__ int s_nan;
    if (tid == 0) s_nan = 0;
    __syncthreads();
    double *kd = reinterpret_cast<double *>(keys);
    int nanc = 0;
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const int e = tid + NT * q;
        double x = __builtin_inf();  // padding sorts after every real value
        if (MODE == 2) {
            x = (double)((e * 2654435761u + i) & 0xFFFFF);
        } else if (e < n) {
            const double t = di + (TR ? dg_in[e] : u_at(U, T_, e, e));
            const double g2 = 2.0 * k2_g<TR>(U, Ut, T_, i, e);
            x = t - g2;
            x = x == 0.0 ? 0.0 : x;  // -0 == +0 (v1's dkey)
            if (x != x) {
                ++nanc;
                x = __builtin_inf();
            }
        }
        kd[V3 ? k2_pad(e) : e] = x;
    }
    if (MODE == 1) {
        if (kd[tid] == 1.2345) scores[i] = kd[tid];  // keep the loads
        return;
    }
    if (nanc) atomicAdd(&s_nan, nanc);
    __syncthreads();
    double dv[KPT];
    if constexpr (V3) {
        k2_get<double, 0>(dv, kd, tid);
    } else {
#pragma unroll
        for (int q = 0; q < KPT; ++q) dv[q] = kd[tid * KPT + q];
    }
    const int64_t nfin = n - s_nan;
    __syncthreads();  // kd[] reads before the sort's writes
    double sum;
    if constexpr (V3) {
        k2_sort16<double>(dv, kd, N, tid);
        sum = k2_sum<double, NT, NT_SUM, true>(kd, k, tid, red, nfin);
    } else {
        k2_sort<double, NT, KPT>(dv, kd, N, tid);
        sum = k2_sum<double, NT, NT_SUM>(kd, k, tid, red, nfin);
    }
    if (tid == 0) scores[i] = (k > 0) ? sum : 0.0;
}

// Ut (the off-diagonal upper tiles transposed) and the contiguous diagonal,
// for K2's coalesced row reads at large n; one 64x64 tile per block through LDS
// [bj0, bj1]: the off-diagonal tiles transposed are those of block-columns
// bj0..bj1 only -- the rows [64 bj0, 64 bj1 + 64) a rank scores under split
// scoring read no others; the diagonal (every row's G_jj) always
__global__ __launch_bounds__(256) void k_transpose(const double *__restrict__ U, int T_,
                                                   double *__restrict__ Ut,
                                                   double *__restrict__ dg, int bj0, int bj1) {
    __shared__ double t[64][65];
    int bi, bj;
    tri_decode(blockIdx.x, T_, bi, bj);
    const double *src = U + (int64_t)blockIdx.x * 4096;
    if (bi == bj) {
        if (threadIdx.x < 64) dg[bi * 64 + threadIdx.x] = src[threadIdx.x * 65];
        return;
    }
    if (bj < bj0 || bj > bj1) return;  // block-uniform
    for (int e = threadIdx.x; e < 4096; e += 256) t[e >> 6][e & 63] = src[e];
    __syncthreads();
    double *dst = Ut + (int64_t)blockIdx.x * 4096;
    for (int e = threadIdx.x; e < 4096; e += 256) dst[e] = t[e & 63][e >> 6];
}

// ---------------------------------------------------------------------------
// K3: rank_i = #{j : key_j < key_i} + #{j < i : key_j == key_i}; mask = rank < m
// ---------------------------------------------------------------------------
// one wave per row: lanes sweep j, a ballot counts the keys ranked before i.
// The ranks are a permutation of 0..n-1, so exactly one row writes each of
// bnd[0] = the highest selected score (rank m-1) and bnd[1] = the lowest
// rejected one (rank m): the selection boundary, for K3b's margin.
__global__ __launch_bounds__(256) void k_rank(const double *__restrict__ scores, int n, int m,
                                              int *__restrict__ mask, double *__restrict__ bnd) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;  // wave-uniform
    const double si = scores[i];
    const uint64_t ki = dkey(si);
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        bool before = false;
        if (j < n) {
            const uint64_t kj = dkey(scores[j]);
            before = (kj < ki) || (kj == ki && j < i);
        }
        cnt += __popcll(__ballot(before));
    }
    if (lane == 0) {
        mask[i] = cnt < m ? 1 : 0;
        if (cnt == m - 1) bnd[0] = si;
        if (cnt == m) bnd[1] = si;
    }
}

// K3b: ascending compaction of mask (single workgroup of 1024 threads), then
// the selection margin (SURVEY.md §7 "Hard parts", §8(d)):
//   gap       = s[rank m] - s[rank m-1]  (lowest rejected - highest selected)
//   err_bound = 2 (e_here + e_ref),  e = 4 k M' (gamma_{d+2}(u_G) + 2 u + gamma_k(u))
// where M' = max finite G_ii (1 + 2 gamma_{d+2}(u_G)) bounds max ||x_i||^2, u =
// 2^-53 (the distance and score arithmetic, and numpy's BLAS Gram), u_G the
// Gram's unit roundoff here (2^-53; 2^-24 on the fp32 MFMA), d = the Gram's
// column count (carried in the packed upper's trailing element, so it is the
// TOTAL d after a multi-GPU exchange).  Every computed score lies within e of
// the exact one, so whenever gap > err_bound the reference selects exactly this
// set; otherwise near_tie = 1 (also for exact ties, e.g. k = 0).
// margin[0..7] = {gap, err_bound, near_tie, M, s_lo, s_hi, d, k}
__global__ __launch_bounds__(1024) void k_compact(const int *__restrict__ mask, int n,
                                                  int64_t *__restrict__ sel,
                                                  const double *__restrict__ diag,
                                                  const double *__restrict__ bnd,
                                                  const double *__restrict__ dcols, int64_t k,
                                                  double *__restrict__ margin) {
    __shared__ int pre[1024];
    __shared__ double mx[16];
    const int tid = threadIdx.x;
    const int chunk = (n + 1023) / 1024;
    const int c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
    int cnt = 0;
    for (int j = c0; j < c1; ++j) cnt += mask[j];
    pre[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
        const int v = tid >= o ? pre[tid - o] : 0;
        __syncthreads();
        pre[tid] += v;
        __syncthreads();
    }
    int pos = pre[tid] - cnt;
    for (int j = c0; j < c1; ++j)
        if (mask[j]) sel[pos++] = j;
    if (!margin) return;  // block-uniform
    // M = max finite G_ii (NaN / Inf rows have NaN / Inf scores in the
    // reference too: they order last, deterministically)
    double m = 0.0;
    for (int j = tid; j < n; j += 1024) {
        const double v = diag[j];
        if (v == v && v < __builtin_inf() && v > m) m = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) mx[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        double M = 0.0;
        for (int w = 0; w < 16; ++w) M = fmax(M, mx[w]);
        // the packed record's trailing record: the Gram's column count, the
        // part of it accumulated on the fp32 MFMA and the int8-sliced columns'
        // absolute error bound (after an exchange: totals)
        write_margin_rec(margin, bnd[0], bnd[1], M, dcols[0], dcols[1], dcols[2], k);
    }
}

// ===========================================================================
// launchers
// ===========================================================================

static int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

template <int NT, int KPT, int NT_SUM, bool TR>
static void launch_scores2(const double *U, const double *Ut, const double *dg, int T, int n, int N,
                           int64_t k, double *scores, double *diag, hipStream_t st, int r0,
                           int rows) {
    const size_t lds = (size_t)(KPT == 16 ? N + N / 16 : N) * sizeof(uint64_t);  // v3: padded
    if constexpr (kProbes) {  // timing-only ablations (tools/k2_modes.py): probe builds only
        static const int mode = [] {
            const char *e = probe_env("BK_K2_MODE");
            return e ? atoi(e) : 0;
        }();
        if (mode == 1) {
            hipLaunchKernelGGL((k_scores2<NT, KPT, NT_SUM, TR, 1>), dim3(rows), dim3(NT), lds, st,
                               U, Ut, dg, T, n, N, k, scores, diag, r0);
            return;
        }
        if (mode == 2) {
            hipLaunchKernelGGL((k_scores2<NT, KPT, NT_SUM, TR, 2>), dim3(rows), dim3(NT), lds, st,
                               U, Ut, dg, T, n, N, k, scores, diag, r0);
            return;
        }
    }
    hipLaunchKernelGGL((k_scores2<NT, KPT, NT_SUM, TR>), dim3(rows), dim3(NT), lds, st, U, Ut, dg,
                       T, n, N, k, scores, diag, r0);
}

bool scores_transposed(int n) {
    static const int tmin = [] {
        const char *e = probe_env("BK_K2_TRANSPOSE_MIN_N");  // probe knob
        return e ? atoi(e) : 2049;
    }();
    return n >= tmin;
}

hipError_t launch_transpose(const double *U, int T, double *Ut, double *dg, hipStream_t st,
                            int bj0, int bj1) {
    if (bj1 < 0) bj1 = T - 1;
    hipLaunchKernelGGL(k_transpose, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st, U, T, Ut,
                       dg, bj0, bj1);
    return hipGetLastError();
}

// The k_scores2 shapes, X(NT, KPT, NT_SUM, when): launch_scores takes the first
// whose `when` holds for the N keys of a row (a power of two, 256 at least);
// the v1 summation shape (NT_SUM = 256 / 1024 threads) is emulated.
// Up to 2048 keys: 256 threads, KPT = N / 256, from the packed tiles only
#define BK_K2_SMALL_SHAPES(X)  \
    X(256, 1, 256, N == 256)   \
    X(256, 2, 256, N == 512)   \
    X(256, 4, 256, N == 1024)  \
    X(256, 8, 256, N == 2048)
// above that, and whenever the rows come from Ut: KPT = 16 (4 at 4096 keys
// under the probe knob BK_K2_KPT).  configure_scores_kernels raises the
// dynamic-LDS limit of these
#define BK_K2_BIG_SHAPES(X)                      \
    X(1024, 4, 1024, N == 4096 && kpt_big == 4)  \
    X(256, 16, 1024, N == 4096)                  \
    X(512, 16, 1024, N == 8192)                  \
    X(1024, 16, 1024, true)

hipError_t launch_scores(const double *U, const double *Ut, const double *dg, int T, int n,
                         int64_t k, double *scores, double *diag, hipStream_t st, int r0,
                         int rows) {
    if (rows < 0) rows = n - r0;
    if (r0 < 0 || rows < 0 || r0 + rows > n) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const int np2 = next_pow2(n < 2 ? 2 : n);
    static const int kpt_big = [] {  // probe knob: keys per thread above 2048 keys
        const char *e = probe_env("BK_K2_KPT");
        return e ? atoi(e) : 16;
    }();
    const int N = np2 < 256 ? 256 : np2;
#define BK_K2_TRY(NT, KPT, NS, WHEN, TR)                                                     \
    if (WHEN) {                                                                              \
        launch_scores2<NT, KPT, NS, TR>(U, Ut, dg, T, n, N, k, scores, diag, st, r0, rows);  \
        return hipGetLastError();                                                            \
    }
#define BK_K2_PACKED(NT, KPT, NS, WHEN) BK_K2_TRY(NT, KPT, NS, WHEN, false)
#define BK_K2_TRANSPOSED(NT, KPT, NS, WHEN) BK_K2_TRY(NT, KPT, NS, WHEN, true)
    if (Ut) {
        BK_K2_BIG_SHAPES(BK_K2_TRANSPOSED)
    }
    BK_K2_SMALL_SHAPES(BK_K2_PACKED)
    BK_K2_BIG_SHAPES(BK_K2_PACKED)
#undef BK_K2_TRANSPOSED
#undef BK_K2_PACKED
#undef BK_K2_TRY
}

hipError_t launch_rank(const double *scores, int n, int m, int *mask, double *bnd,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_rank, dim3((n + 3) / 4), dim3(256), 0, st, scores, n, m, mask, bnd);
    return hipGetLastError();
}

// split scoring (bk_api.hip stage_finish): the gathered slices {ch scores,
// status} of `parts` ranks -> the n scores, contiguous; rec = the Gram's
// trailing record dcols[0..2], or NaN words when any rank's status is not 0
__global__ __launch_bounds__(256) void k_split_unpack(const double *__restrict__ sg, int64_t ch,
                                                      int parts, int n,
                                                      const double *__restrict__ dcols,
                                                      double *__restrict__ scores,
                                                      double *__restrict__ rec) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n) scores[i] = sg[i + i / ch];
    if (blockIdx.x != 0) return;
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int p = (int)threadIdx.x; p < parts; p += 256)
        if (sg[(int64_t)p * (ch + 1) + ch] != 0.0) bad = 1;  // NaN compares unequal too
    __syncthreads();
    if (threadIdx.x < 3) rec[threadIdx.x] = bad ? __builtin_nan("") : dcols[threadIdx.x];
}

hipError_t launch_split_unpack(const double *sg, int64_t ch, int parts, int n, const double *dcols,
                               double *scores, double *rec, hipStream_t st) {
    hipLaunchKernelGGL(k_split_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sg, ch,
                       parts, n, dcols, scores, rec);
    return hipGetLastError();
}

hipError_t launch_compact(const int *mask, int n, int64_t *sel, const double *diag,
                          const double *bnd, const double *dcols, int64_t k, double *margin,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, mask, n, sel, diag, bnd, dcols, k,
                       margin);
    return hipGetLastError();
}

hipError_t configure_scores_kernels() {
#ifdef BK_PROBES  // with the timing-only K2 ablations (BK_K2_MODE)
#define BK_K2_MODES(NT, KPT, NS, TR)                                                      \
    (const void *)k_scores2<NT, KPT, NS, TR>, (const void *)k_scores2<NT, KPT, NS, TR, 1>, \
        (const void *)k_scores2<NT, KPT, NS, TR, 2>,
#else
#define BK_K2_MODES(NT, KPT, NS, TR) (const void *)k_scores2<NT, KPT, NS, TR>,
#endif
#define BK_K2_BOTH(NT, KPT, NS, WHEN) BK_K2_MODES(NT, KPT, NS, false) BK_K2_MODES(NT, KPT, NS, true)
    for (const void *k : {BK_K2_BIG_SHAPES(BK_K2_BOTH)}) {
        // v3 at N = 16384: 136 KiB
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (e != hipSuccess) return e;
    }
#undef BK_K2_BOTH
#undef BK_K2_MODES
    return hipSuccess;
}

}  // namespace bk
