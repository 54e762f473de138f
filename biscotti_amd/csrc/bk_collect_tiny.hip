// bk_collect_tiny.hip -- the incremental collection of a TINY round in ONE
// workgroup (include/bk.h bk_set_collect_tiny): at most 16 rows collected, d <=
// 128 (config A, creditcard: 10 x 25; a real localTest verifier sees n <= 4).
//
// k_tiny's reasoning (bk_small_items.h tiny_body) applied to the collection:
// at this shape the hand-offs between workgroups and the row's copy ARE the
// cost of k_collect_arrive, and the whole state -- 16 rows of
// at most 1 KiB, a 16 x 16 Gram -- fits one workgroup's LDS.  k_collect_tiny is
// a grid of 1 with 256 threads, no queue, no flags, no time-out word, and up to
// three steps separated by workgroup barriers:
//
//   arrival  the cnt new rows are read where they are -- host rows in the
//            collection's mapped pinned arrival block (the CPU memcpy'd them
//            there; the loads cross PCIe as k_tiny's of a pinned batch do),
//            device rows through the pointers in the launch arguments -- one
//            element per thread, so any 8-byte (fp32: 4-byte) aligned row will
//            do.  NOISED: the row is delta[c] + ((0 + v_0[c]) + .. + v_{k-1}[c])
//            / k, k_collect_noise's order and bits.  The row goes to LDS and, the
//            columns below d only, to its store row (the pad columns [d, ld)
//            are bk_collect_begin's zeros and stay).  The resident rows come
//            from the store by 16-B loads, the resident Gram runs from G.
//   border   one wave per element G[j (j + 1) / 2 + i], i <= j, j a new slot:
//            k_border + k_border_reduce's sum (arrive_border in
//            bk_arrive_items.h restates it).  A row of this range is one chunk
//            and vector l of it belongs to lane l, so the lane's eight loads
//            are this vector and seven masked (zero) ones: one fma per element
//            from +0.0, then the seven fma(0, 0, acc) as the single acc + 0.0
//            they amount to (they only turn a -0.0 into +0.0), the vector's
//            elements added in order, the xor butterfly 32..1; the reduce adds
//            the one chunk partial to 0.0, and its butterfly adds +0.0 only.
//            The element is kept in LDS and stored to G.
//   finish   (when asked) tiny_body's scores, selection, margin and mean on the
//            Gram in LDS read through the order: small_rank_sum's distances, a
//            sort by counting, K2's summation shape (lane t adds rank 1 + t, the
//            wave butterfly, the four waves' sums in order -- waves 1-3 hold
//            +0.0 at n <= 16), the (score, index) rank, the mean's adds in
//            ascending selected order from the rows in LDS.  Outputs go to the
//            context's mapped output block.
//
// Nothing the launch wrote to global memory is read back from it: new rows and
// their Gram runs are consumed from LDS.  Everything an earlier launch wrote
// (store rows, Gram runs) is ordered before this launch by the stream.
#include "bk_small_items.h"

namespace bk {

namespace {

typedef float tf4 __attribute__((ext_vector_type(4)));
template <typename T>
struct TinyVec;
template <>
struct TinyVec<double> {
    typedef d2v type;
    static constexpr int N = 2;
};
template <>
struct TinyVec<float> {
    typedef tf4 type;
    static constexpr int N = 4;
};

constexpr int TN = COLLECT_TINY_MAX_N;         // rows, and the side of the Gram in LDS
constexpr int TROW = COLLECT_TINY_SLOT_BYTES;  // bytes of a staged row
static_assert(COLLECT_TINY_MAX_D * 8 == TROW, "a row of the range fills a slot at most");
static_assert(TROW / 16 == 64, "vector l of a row belongs to lane l of the border's wave");
static_assert(TROW <= COLLECT_BORDER_CHUNK_BYTES, "one border chunk per row");

struct CollectTinyArgs {
    void *store;  // the row store (ld elements per row)
    double *G;    // the Gram by arrival slot, lower packed
    int64_t ld, d;
    const void *src[TN];  // the cnt new rows (NOISED: src[0] is the delta)
    int j0, cnt;          // rows resident before the launch; rows arriving in it
    int fin, n, f;        // fin: the finish of n rows through order
    uint8_t order[TN];    // entries past n are 0
    int64_t *sel;
    double *mean, *margin, *scores_out;
};

struct CollectTinyNoisedArgs {
    CollectTinyArgs a;
    const double *vec[COLLECT_ARRIVE_NOISE_MAX_K];  // the k noise vectors of the one new row
    int k;
};

template <bool NOISED>
struct TinyArgsOf {
    typedef CollectTinyArgs type;
};
template <>
struct TinyArgsOf<true> {
    typedef CollectTinyNoisedArgs type;
};

__device__ __forceinline__ const CollectTinyArgs &tiny_base(const CollectTinyArgs &a) { return a; }
__device__ __forceinline__ const CollectTinyArgs &tiny_base(const CollectTinyNoisedArgs &a) {
    return a.a;
}

// element c of the one new row of a noised launch: k_collect_noise's sum, eight
// loads in flight
__device__ __forceinline__ double tiny_noised(const CollectTinyNoisedArgs &na, int c) {
    const int k = na.k;
    double sum = 0.0;
    int j = 0;
    for (; j + 8 <= k; j += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = __builtin_nontemporal_load(na.vec[j + q] + c);
#pragma unroll
        for (int q = 0; q < 8; ++q) sum += v[q];
    }
    for (; j < k; ++j) sum += __builtin_nontemporal_load(na.vec[j] + c);
    const double x = __builtin_nontemporal_load((const double *)na.a.src[0] + c);
    return x + sum / (double)k;
}

}  // namespace

template <typename T, bool NOISED>
__global__ __launch_bounds__(256) void k_collect_tiny(typename TinyArgsOf<NOISED>::type ka) {
    static_assert(!NOISED || sizeof(T) == 8, "noise is fp64 only");
    typedef typename TinyVec<T>::type V;
    constexpr int N = TinyVec<T>::N;
    __shared__ __attribute__((aligned(16))) char rows[TN * TROW];  // row r at r TROW, as T
    __shared__ double gm[TN * TN];       // gm[h TN + l] = G[h (h + 1) / 2 + l], l <= h
    __shared__ uint64_t keys[4][TN];     // each wave's row keys
    __shared__ double srt[4][TN];        // each wave's sorted row
    __shared__ double scs[TN];
    __shared__ uint64_t skey[TN];
    __shared__ double bnd[2];
    __shared__ uint64_t balw;
    __shared__ int sord[TN];
    const CollectTinyArgs &a = tiny_base(ka);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j0 = a.j0, cnt = a.cnt;
    const int ld = (int)a.ld, d = (int)a.d;
    T *store = (T *)a.store;

    // ---- arrival
    if (tid < TN) sord[tid] = (int)a.order[tid];
    {
        // the resident Gram runs
        const int h = tid >> 4, l = tid & 15;
        if (h < j0 && l <= h) gm[h * TN + l] = a.G[h * (h + 1) / 2 + l];
        // the resident rows, whole 16-B vectors (the pad columns are zero)
        const int nvec = ld / N;
        for (int v = tid; v < j0 * 64; v += 256) {
            const int r = v >> 6, q = v & 63;
            if (q < nvec)
                reinterpret_cast<V *>(rows + r * TROW)[q] =
                    reinterpret_cast<const V *>(store + (int64_t)r * ld)[q];
        }
        // the new rows: thread (rr, c) takes column c of rows rr, rr + 2, ..
        const int c = tid & 127, rr = tid >> 7;
        if constexpr (NOISED) {
            if (rr == 0 && c < ld) {
                double x = 0.0;
                if (c < d) {
                    x = tiny_noised(ka, c);
                    store[(int64_t)j0 * ld + c] = x;
                }
                reinterpret_cast<double *>(rows + j0 * TROW)[c] = x;
            }
        } else {
            T x[TN / 2];
#pragma unroll
            for (int u = 0; u < TN / 2; ++u) {
                const int r = rr + 2 * u;
                x[u] = (T)0;
                if (r < cnt && c < d) x[u] = __builtin_nontemporal_load((const T *)a.src[r] + c);
            }
#pragma unroll
            for (int u = 0; u < TN / 2; ++u) {
                const int r = rr + 2 * u;
                if (r < cnt && c < ld) {
                    reinterpret_cast<T *>(rows + (j0 + r) * TROW)[c] = x[u];
                    if (c < d) store[(int64_t)(j0 + r) * ld + c] = x[u];
                }
            }
        }
    }
    __syncthreads();

    // ---- border: element p of the new runs, slot j0's first, to wave p % 4
    {
        const int np = cnt * j0 + cnt * (cnt + 1) / 2;
        for (int p = wave; p < np; p += 4) {
            int j = j0, i = p;
            while (i > j) {
                i -= j + 1;
                ++j;
            }
            V x = {}, y = {};
            if (lane * N < d) {  // whole 16-B vectors: the pad columns are 0
                x = reinterpret_cast<const V *>(rows + i * TROW)[lane];
                y = reinterpret_cast<const V *>(rows + j * TROW)[lane];
            }
            double acc[N];
#pragma unroll
            for (int e = 0; e < N; ++e) {
                acc[e] = __builtin_fma((double)x[e], (double)y[e], 0.0);
                acc[e] = acc[e] + 0.0;  // the lane's seven masked vectors: fma(0, 0, acc)
            }
            double v = acc[0];
#pragma unroll
            for (int e = 1; e < N; ++e) v += acc[e];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) {
                // k_border_reduce on one chunk: 0.0 + the partial (its butterfly
                // then adds +0.0 to a value that is not -0.0)
                const double g = 0.0 + v;
                gm[j * TN + i] = g;
                a.G[j * (j + 1) / 2 + i] = g;
            }
        }
    }
    if (!a.fin) return;
    __syncthreads();

    // ---- finish: tiny_body on the Gram read through the order
    const int n = a.n, m = n - a.f;
    const int64_t k = n - a.f - 2 > 0 ? n - a.f - 2 : 0;
    const int ol = sord[lane & 15];
    for (int i = wave; i < n; i += 4) {
        const int oi = sord[i];
        const double di = gm[oi * TN + oi];
        uint64_t key = ~0ULL;  // padding sorts last
        if (lane < n) {
            const int hi = oi > ol ? oi : ol, lo = oi > ol ? ol : oi;
            key = dkey((di + gm[ol * TN + ol]) - 2.0 * gm[hi * TN + lo]);
        }
        if (lane < TN) keys[wave][lane] = key;
        __builtin_amdgcn_wave_barrier();
        int c = 0;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const uint64_t o = keys[wave][j];
            c += (o < key) || (o == key && j < lane);
        }
        if (lane < TN) srt[wave][c] = dkey_inv(key);
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        if (1 + lane <= k) acc += srt[wave][1 + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) {
            double sum = 0.0;  // the four waves' sums in order (waves 1-3: +0.0)
            sum += acc;
            sum += 0.0;
            sum += 0.0;
            sum += 0.0;
            scs[i] = k > 0 ? sum : 0.0;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (tid < TN) skey[tid] = tid < n ? dkey(scs[tid]) : ~0ULL;
    __syncthreads();
    if (wave == 0) {
        bool on = false;
        if (lane < n) {
            const uint64_t ki = skey[lane];
            int c = 0;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const uint64_t o = skey[j];
                c += (o < ki) || (o == ki && j < lane);
            }
            on = c < m;
            if (c == m - 1) bnd[0] = scs[lane];
            if (c == m) bnd[1] = scs[lane];
            if (a.scores_out) a.scores_out[lane] = scs[lane];
        }
        const uint64_t bal = __ballot(on);
        if (on) a.sel[__popcll(bal & ((1ull << lane) - 1))] = (int64_t)lane;
        if (lane == 0) balw = bal;
    }
    __syncthreads();
    if (tid == 0) {
        double M = 0.0;
        for (int j = 0; j < n; ++j) {
            const double v = gm[sord[j] * TN + sord[j]];
            if (v == v && v < __builtin_inf() && v > M) M = v;
        }
        write_margin(a.margin, bnd[0], bnd[1], M, (double)a.d, k, 0x1p-53);
    }
    if (a.mean && tid < d) {
        // column tid, the caller's rows in ascending order, each row's value or
        // +0.0 by the selection mask (acc is never -0.0: k_small's M items)
        const uint64_t sb = balw;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < TN; ++r) {
            const double v = (double)reinterpret_cast<const T *>(rows + sord[r] * TROW)[tid];
            acc += ((sb >> r) & 1) ? v : 0.0;
        }
        a.mean[tid] = acc / (double)m;
    }
}

hipError_t launch_collect_tiny(const CollectTinyLaunch &L, hipStream_t st) {
    const int after = L.j0 + L.cnt;
    if (L.j0 < 0 || L.cnt < 0 || after < 1 || after > TN || L.d < 1 || L.d > COLLECT_TINY_MAX_D ||
        L.ld < L.d || L.ld * (L.dtype == 0 ? 8 : 4) > TROW || !L.store || !L.G)
        return hipErrorInvalidValue;
    if (L.k < 0 || L.k > COLLECT_ARRIVE_NOISE_MAX_K || (L.k > 0 && (L.cnt != 1 || L.dtype != 0)))
        return hipErrorInvalidValue;
    if (!L.fin && L.cnt == 0) return hipErrorInvalidValue;
    CollectTinyNoisedArgs na = {};
    CollectTinyArgs &a = na.a;
    a.store = L.store;
    a.G = L.G;
    a.ld = L.ld;
    a.d = L.d;
    a.j0 = L.j0;
    a.cnt = L.cnt;
    for (int r = 0; r < L.cnt; ++r) {
        if (!L.src[r]) return hipErrorInvalidValue;
        a.src[r] = L.src[r];
    }
    if (L.fin) {
        if (L.n < 1 || L.n > after || L.f < 1 || L.f >= L.n || !L.sel || !L.margin)
            return hipErrorInvalidValue;
        a.fin = 1;
        a.n = L.n;
        a.f = L.f;
        for (int i = 0; i < L.n; ++i) {
            const int64_t o = L.order ? L.order[i] : i;
            if (o < 0 || o >= after) return hipErrorInvalidValue;
            a.order[i] = (uint8_t)o;
        }
        a.sel = L.sel;
        a.mean = L.mean;
        a.margin = L.margin;
        a.scores_out = L.scores_out;
    }
    if (L.k > 0) {
        na.k = L.k;
        for (int q = 0; q < L.k; ++q) {
            if (!L.vecs || !L.vecs[q]) return hipErrorInvalidValue;
            na.vec[q] = L.vecs[q];
        }
        hipLaunchKernelGGL((k_collect_tiny<double, true>), dim3(1), dim3(256), 0, st, na);
    } else if (L.dtype == 0) {
        hipLaunchKernelGGL((k_collect_tiny<double, false>), dim3(1), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_collect_tiny<float, false>), dim3(1), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace bk
