// bk_collect.hip -- incremental Multi-Krum (include/bk.h bk_collect_*): the
// verifier's updates arrive one RPC at a time (VerifyUpdateKRUM, krum.go:227-365),
// so each row is uploaded and folded into the Gram when it arrives, and only
// the scores, the selection and the mean remain after the last arrival.
//
// Per collection (one per context, all on the context stream):
//   store   n_cap x ld rows in the input dtype, 16-B aligned rows, pad columns 0
//   G       the Gram by arrival slot, fp64, lower-triangular packed: row j holds
//           G[j][0..j] at j (j + 1) / 2, so an arrival writes one contiguous run
//   ring    a small pinned ring through which pageable rows cross PCIe
// Kernels:
//   k_border         <x_i, x_j> partials of up to BORDER_ROWS new slots j against
//                    every slot i <= j, per chunk of BORDER_CHUNK_BYTES of a row
//   k_border_reduce  the chunks' partials summed in a fixed order -> G
//   k_collect_gather G, through the caller's order -> the packed upper + record
//   k_collect_selmap the selection mapped to arrival slots, for K4 on the store
// A finish of n <= 128 rows, d <= 32,768 (small_ok) takes none of the last two
// nor K2..K4: one k_collect_small launch (bk_small.hip) does it all, and
// bk_collect_finish_batch runs many such finishes over the one collection as
// k_collect_small_batch launches (bk_collect_batch.hip), and
// bk_collect_finish_ragged, where every problem has its own n and f, as
// k_collect_small_ragged launches (bk_collect_ragged.hip).  With
// bk_set_collect_wide on, n <= 128 and 32,768 < d <= BK_COLLECT_WIDE_MAX_D take
// one launch too: k_collect_wide, and k_collect_wide_ragged for the batched and
// ragged entries (bk_collect_wide.hip).
// bk_collect_add_noised takes an update as Delta and Noise: k_collect_noise
// (bk_collect_noise.hip) adds the mean of the noise vectors to the arriving
// rows in the store, one launch per group of up to BORDER_ROWS, before the
// same border.
// bk_collect_add_finish is the add of one row and the finish in one call; in
// k_collect_small's range with at most 128 rows collected it is the row's copy
// and ONE launch, k_collect_arrive (bk_collect_arrive.hip): that row's border,
// bit for bit k_border + k_border_reduce's, in front of k_collect_small's items.
// With bk_set_collect_wide_arrive on (and the wide path) a pinned or device row
// in k_collect_wide's range takes ONE launch too: k_collect_arrive_wide
// (bk_collect_arrive_wide.hip), whose border partials meet in P.
// bk_collect_add_noised_finish is that for an update that arrives as Delta and
// Noise: the copies and ONE launch, k_collect_arrive_noised
// (bk_collect_arrive_noised.hip), which noises the new row in front of the
// border.
// With bk_set_collect_tiny on, a collection of at most 16 rows with d <= 128
// runs every add, finish and fused arrival as ONE launch of one workgroup,
// k_collect_tiny (bk_collect_tiny.hip), with no copy call: host rows reach the
// kernel through the collection's mapped pinned arrival block, device rows are
// read where they are.  The store rows and the Gram runs are left as the paths
// above leave them, so the two mix freely.
// Every element of G is the same sum whatever the add's count and however many
// rows are resident: chunk s covers the same columns, one wave sums a chunk's
// products in lane order and the chunks are added in the same tree, so the
// order depends on (d, dtype) alone.  No atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "bk_ctx.h"

using namespace bk;

namespace {

constexpr int BORDER_ROWS = 8;            // new rows per k_border launch (their chunks in LDS)
constexpr int BORDER_CHUNK_BYTES = 8192;  // of one row per workgroup: 64 lanes x 8 loads x 16 B
constexpr int BORDER_VPL = BORDER_CHUNK_BYTES / 16 / 64;  // 16-B loads per lane per row
static_assert(BORDER_CHUNK_BYTES == COLLECT_BORDER_CHUNK_BYTES,
              "k_collect_arrive's B items sum the chunks k_border does");
constexpr size_t RING_SLOT_BYTES = (size_t)1 << 20;
constexpr int RING_SLOTS = 8;
// bk_collect_add_finish: a pageable row longer than this takes the add and the
// finish inside the call, not the fused launch -- at 62,800 B (100 x 7,850) the
// fused call measured no faster than the sequence from pageable memory, at
// 200 B it did; nothing was measured in between
constexpr size_t ARRIVE_HOST_MAX_BYTES = 32768;
// bk_collect_add_noised_finish: host rows longer than this take the noised add
// and the finish inside the call, not the fused launch, but for pinned rows with
// k = 1.  At 62,800 B (100 x 7,850) the fused call's runs were all below the
// sequence's only there and from pageable memory with k = 2; pinned k = 2 and
// pageable k = 1 overlapped by one run each.  At 200 B every setting was ahead
// (DESIGN 5o); nothing was measured in between.  Device rows are fused at
// every d of the range
constexpr size_t ARRIVE_NOISED_HOST_MAX_BYTES = 32768;
// bk_set_collect_wide_arrive(ctx, 1): the fused wide launch is taken only for a
// pinned row of at most this many bytes in a call that asks for the mean -- at
// 100 x 40,000 fp64 that call's three runs were all below the sequence's (88.0
// [87.5 .. 89.1] against 89.8 [89.4 .. 90.7] us); without the mean they
// overlapped (51.0 [49.7 .. 53.7] against 55.3 [50.7 .. 55.8]), device rows were
// level (40.6 against 39.7), and at 100 x 163,850 and 100 x 259,770 the fused
// call was level or behind in every setting (fp64 device rows without the mean:
// 58.3 against 54.3, 73.9 against 68.6 us).  Nothing was measured in
// between.  on = 2 takes the launch in the whole range (tests, measurements)
constexpr size_t ARRIVE_WIDE_MAX_BYTES = 320000;

typedef double cd2 __attribute__((ext_vector_type(2)));
typedef float cf4 __attribute__((ext_vector_type(4)));
template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
    typedef cd2 type;
    static constexpr int N = 2;
};
template <>
struct Vec16<float> {
    typedef cf4 type;
    static constexpr int N = 4;
};

// grid (S chunks, row blocks of rpb rows), 256 threads.  Chunk s = columns
// [s KC, s KC + KC), KC = BORDER_CHUNK_BYTES / sizeof(T).  The C new rows'
// chunks sit in LDS (C x 8 KiB); each wave streams one resident (or new) row i
// of its block straight into registers, 8 x 16 B per lane, and keeps C x N fp64
// accumulators: element e of load t multiplies the new row's element of the
// same column (fp32 widened: the product is exact) and is added by one fma, t
// ascending; the N accumulators are added in order, then the 64 lanes by a
// xor butterfly (32, 16, .., 1).  P[(s C + c) jend + i] = the chunk's partial
// of <x_i, x_{j0 + c}>, written for i <= j0 + c < jend only.
template <typename T, int C>
__global__ __launch_bounds__(256) void k_border(const T *__restrict__ store, int64_t ld, int64_t d,
                                                int j0, int jend, int rpb,
                                                double *__restrict__ P) {
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
    constexpr int VPC = BORDER_CHUNK_BYTES / 16;  // 16-B vectors per row chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char border_lds[];
    V *lv = reinterpret_cast<V *>(border_lds);
    const int tid = threadIdx.x, s = blockIdx.x;
    const int64_t c0 = (int64_t)s * (VPC * N);
    for (int v = tid; v < C * VPC; v += 256) {
        const int c = v / VPC, q = v % VPC;
        const int jr = j0 + c < jend ? j0 + c : jend - 1;  // a launch of fewer than C rows
        const int64_t col = c0 + (int64_t)q * N;
        V x = {};
        if (col < d) x = *reinterpret_cast<const V *>(store + (int64_t)jr * ld + col);
        lv[v] = x;
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63;
    const int r0 = (int)blockIdx.y * rpb;
    const int r1 = r0 + rpb < jend ? r0 + rpb : jend;
    for (int i = r0 + w; i < r1; i += 4) {
        const T *row = store + (int64_t)i * ld + c0;
        V x[BORDER_VPL];
#pragma unroll
        for (int t = 0; t < BORDER_VPL; ++t) {
            const int q = t * 64 + lane;
            V z = {};
            x[t] = c0 + (int64_t)q * N < d
                       ? __builtin_nontemporal_load(reinterpret_cast<const V *>(row) + q)
                       : z;
        }
        double acc[C][N];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int e = 0; e < N; ++e) acc[c][e] = 0.0;
        // C = 1: the new row's chunk stays in registers across the rows (the
        // LDS reads hoist); more new rows would take C x 32 registers and the
        // occupancy with them, so their reads stay in the loop
        int ll = lane;
        if constexpr (C > 1) asm volatile("" : "+v"(ll));
#pragma unroll
        for (int t = 0; t < BORDER_VPL; ++t)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const V y = lv[c * VPC + t * 64 + ll];
#pragma unroll
                for (int e = 0; e < N; ++e)
                    acc[c][e] = __builtin_fma((double)x[t][e], (double)y[e], acc[c][e]);
            }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double v = acc[c][0];
#pragma unroll
            for (int e = 1; e < N; ++e) v += acc[c][e];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == c && j0 + c < jend && i <= j0 + c)
                P[((int64_t)s * C + c) * jend + i] = v;
        }
    }
}

// one wave per element (c, i), i <= j0 + c: lane l adds the partials of chunks
// l, l + 64, .. in that order, then the lanes by the same butterfly -> G
__global__ __launch_bounds__(256) void k_border_reduce(const double *__restrict__ P, int S, int C,
                                                       int j0, int jend, double *__restrict__ G) {
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= (int64_t)(jend - j0) * jend) return;  // wave-uniform
    const int c = (int)(item / jend), i = (int)(item % jend);
    const int j = j0 + c;
    if (i > j) return;
    double v = 0.0;
    for (int s = lane; s < S; s += 64) v += P[((int64_t)s * C + c) * jend + i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) G[(int64_t)j * (j + 1) / 2 + i] = v;
}

// The packed upper of the caller's rows 0..n-1 (bk_upper_elems(n): 64x64
// sub-tiles, diagonal tiles valid for ir <= ic; the rest 0) from G through
// order (row a of the caller = arrival slot order[a]), and the trailing
// record {d, 0, 0, 0}.  One sub-tile per workgroup.
__global__ __launch_bounds__(256) void k_collect_gather(const double *__restrict__ G,
                                                        const int64_t *__restrict__ order, int n,
                                                        int T, double dcols,
                                                        double *__restrict__ U) {
    __shared__ int64_t so[128];
    int br = 0, rem = (int)blockIdx.x;
    while (rem >= T - br) {
        rem -= T - br;
        ++br;
    }
    const int bc = br + rem;
    if (threadIdx.x < 128) {
        const int r = (threadIdx.x < 64 ? br * 64 : bc * 64 - 64) + (int)threadIdx.x;
        so[threadIdx.x] = r < n ? order[r] : -1;
    }
    __syncthreads();
    double *tile = U + (int64_t)blockIdx.x * 4096;
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int ir = e >> 6, ic = e & 63;
        const int64_t oa = so[ir], ob = so[64 + ic];
        double v = 0.0;
        if (oa >= 0 && ob >= 0 && (br < bc || ir <= ic)) {
            const int64_t hi = oa > ob ? oa : ob, lo = oa > ob ? ob : oa;
            v = G[hi * (hi + 1) / 2 + lo];
        }
        tile[e] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < BK_UPPER_TRAIL)
        U[(int64_t)T * (T + 1) / 2 * 4096 + threadIdx.x] = threadIdx.x == 0 ? dcols : 0.0;
}

// K4 reads the row store: its sel list is the selection (the caller's row
// indices, ascending) mapped to arrival slots, in the same order
__global__ __launch_bounds__(256) void k_collect_selmap(const int64_t *__restrict__ sel,
                                                        const int64_t *__restrict__ order, int m,
                                                        int64_t *__restrict__ slots) {
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r < m) slots[r] = order[sel[r]];
}

template <typename T>
hipError_t launch_border_t(const T *store, int64_t ld, int64_t d, int j0, int cnt, int S, int rpb,
                           int RB, double *P, hipStream_t st) {
    const dim3 grid((unsigned)S, (unsigned)RB), block(256);
    const int jend = j0 + cnt;
#define BK_BORDER(C)                                                                        \
    hipLaunchKernelGGL((k_border<T, C>), grid, block, (size_t)(C) * BORDER_CHUNK_BYTES, st, \
                       store, ld, d, j0, jend, rpb, P)
    if (cnt == 1)
        BK_BORDER(1);
    else if (cnt == 2)
        BK_BORDER(2);
    else if (cnt <= 4)
        BK_BORDER(4);
    else
        BK_BORDER(8);
#undef BK_BORDER
    return hipGetLastError();
}

int border_c(int cnt) { return cnt == 1 ? 1 : cnt == 2 ? 2 : cnt <= 4 ? 4 : 8; }

struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
};

}  // namespace

namespace bk {

struct Collect {
    bool begun = false;
    int dtype = BK_F64;
    int64_t n_cap = 0, d = 0, ld = 0, count = 0;
    int S = 0;  // chunks of a row: ceil(d es / BORDER_CHUNK_BYTES)
    // bk_collect_stats, since the begin: k_border launches, k_border_reduce
    // launches, one-launch finishes, fused arrive launches
    int64_t stats[4] = {0, 0, 0, 0};
    Buf store, G, P, U, sel, slots, scores, mean, mean_part, order, horder, ring;
    // bk_collect_finish_batch and bk_collect_finish_ragged: buffers of their
    // own (a single finish or any bk_multikrum* between two such finishes
    // touches none of them; both entries are synchronous, so neither finds the
    // other's work in them): the 16-bit orders (the ragged entry: descriptors,
    // segment starts, then the orders) and their pinned staging, per-problem
    // scores, diag, sel and mean, and the queue lines (zeroed at allocation;
    // every launch leaves them zero).  The records go to the context's batch
    // record store
    Buf b_order, b_horder, b_scores, b_diag, b_sel, b_mean, b_ctr;
    // bk_collect_add_noised: the device staging of a launch's noise vectors
    // (host rows) and the pointer table of a call's device rows with its pinned
    // staging, grown on demand
    Buf nstage, ntab, hntab;
    hipEvent_t ev_slot[RING_SLOTS] = {};
    bool slot_used[RING_SLOTS] = {};
    int ring_next = 0;
    hipEvent_t ev_up = nullptr;
    // bk_set_collect_tiny: the launches of k_collect_tiny since the begin (adds,
    // finishes, adds with a finish) and the arrival block -- mapped pinned host
    // memory the kernel reads over PCIe, TINY_SLOTS slots indexed by arrival
    // slot, each a row and BK_COLLECT_NOISE_MAX_K noise vectors of
    // COLLECT_TINY_SLOT_BYTES.  A slot is written once per collected row, before
    // the launch that reads it; it is written again only after a failed call
    // (which drains the stream) or the next begin (which waits for it)
    int64_t tiny_stats[3] = {0, 0, 0};
    char *arrive = nullptr, *arrive_dev = nullptr;
};

// the batched finish's buffers (the stream is idle)
static void collect_batch_release(Collect *k) {
    for (Buf *b : {&k->b_order, &k->b_horder, &k->b_scores, &k->b_diag, &k->b_sel, &k->b_mean,
                   &k->b_ctr}) {
        if (b->p) (void)(b->pinned ? hipHostFree(b->p) : hipFree(b->p));
        b->p = nullptr;
        b->bytes = 0;
    }
}

void collect_destroy(Collect *k) {
    if (!k) return;
    for (Buf *b : {&k->store, &k->G, &k->P, &k->U, &k->sel, &k->slots, &k->scores, &k->mean,
                   &k->mean_part, &k->order, &k->horder, &k->ring, &k->nstage, &k->ntab, &k->hntab})
        if (b->p) (void)(b->pinned ? hipHostFree(b->p) : hipFree(b->p));
    collect_batch_release(k);
    if (k->arrive) (void)hipHostFree(k->arrive);
    for (hipEvent_t ev : k->ev_slot)
        if (ev) (void)hipEventDestroy(ev);
    if (k->ev_up) (void)hipEventDestroy(k->ev_up);
    delete k;
}

}  // namespace bk

namespace {

// an error path of add / finish: queued copies may still read the caller's rows
struct Drain {
    hipStream_t st;
    bool armed = true;
    ~Drain() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};

// Grow the buffers in `want` to their sizes, all or nothing: the new blocks are
// allocated first, and only when every one exists are the old ones freed
int grow_all(const std::vector<std::pair<Buf *, size_t>> &want, const char *who = "bk_collect_begin") {
    std::vector<void *> fresh(want.size(), nullptr);
    for (size_t i = 0; i < want.size(); ++i) {
        Buf *b = want[i].first;
        const size_t bytes = want[i].second < 256 ? 256 : want[i].second;
        if (bytes <= b->bytes) continue;
        const hipError_t e = b->pinned ? hipHostMalloc(&fresh[i], bytes, hipHostMallocPortable)
                                       : hipMalloc(&fresh[i], bytes);
        if (e != hipSuccess) {
            for (size_t q = 0; q < i; ++q)
                if (fresh[q]) (void)(want[q].first->pinned ? hipHostFree(fresh[q]) : hipFree(fresh[q]));
            return fail(BK_ENOMEM, "%s: %s(%zu bytes): %s", who,
                        b->pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
        }
    }
    for (size_t i = 0; i < want.size(); ++i) {
        if (!fresh[i]) continue;
        Buf *b = want[i].first;
        if (b->p) (void)(b->pinned ? hipHostFree(b->p) : hipFree(b->p));
        b->p = fresh[i];
        b->bytes = want[i].second < 256 ? 256 : want[i].second;
    }
    return BK_OK;
}

// the border of slots [j0, j0 + cnt): groups of up to BORDER_ROWS new rows, each
// group one k_border over every slot up to its last and one k_border_reduce
int fold_border(Collect *k, int64_t j0, int64_t cnt, int num_cu, hipStream_t st) {
    for (int64_t g0 = j0; g0 < j0 + cnt; g0 += BORDER_ROWS) {
        const int gc = (int)(j0 + cnt - g0 < BORDER_ROWS ? j0 + cnt - g0 : BORDER_ROWS);
        const int jend = (int)g0 + gc;
        // row blocks: enough workgroups to fill the chip, at least one row per wave
        int RB = (4 * num_cu + k->S - 1) / k->S;
        if (RB > (jend + 3) / 4) RB = (jend + 3) / 4;
        if (RB < 1) RB = 1;
        if (RB > 65535) RB = 65535;
        const int rpb = ((jend + RB - 1) / RB + 3) / 4 * 4;
        RB = (jend + rpb - 1) / rpb;
        hipError_t e = k->dtype == BK_F64
                           ? launch_border_t((const double *)k->store.p, k->ld, k->d, (int)g0, gc,
                                             k->S, rpb, RB, (double *)k->P.p, st)
                           : launch_border_t((const float *)k->store.p, k->ld, k->d, (int)g0, gc,
                                             k->S, rpb, RB, (double *)k->P.p, st);
        if (e != hipSuccess) return fail(BK_EHIP, "k_border launch: %s", hipGetErrorString(e));
        ++k->stats[0];
        const int64_t items = (int64_t)gc * jend;
        hipLaunchKernelGGL(k_border_reduce, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st,
                           (const double *)k->P.p, k->S, border_c(gc), (int)g0, jend,
                           (double *)k->G.p);
        e = hipGetLastError();
        if (e != hipSuccess)
            return fail(BK_EHIP, "k_border_reduce launch: %s", hipGetErrorString(e));
        ++k->stats[1];
    }
    return BK_OK;
}

// one pageable row through the pinned ring: the host copy of a piece overlaps
// the DMA of the one before; on return the row is in the ring or on the device.
// record = false (bk_collect_add_finish's fused path, which waits for the
// stream before it returns or fails): no event behind the copy, the slot is
// free again once that wait is over
int upload_pageable(Collect *k, char *dst, const char *src, size_t bytes, hipStream_t st,
                    bool record = true) {
    for (size_t off = 0; off < bytes; off += RING_SLOT_BYTES) {
        const size_t len = bytes - off < RING_SLOT_BYTES ? bytes - off : RING_SLOT_BYTES;
        const int s = k->ring_next;
        k->ring_next = (s + 1) % RING_SLOTS;
        if (k->slot_used[s]) HIPCHK(hipEventSynchronize(k->ev_slot[s]));
        char *slot = (char *)k->ring.p + (size_t)s * RING_SLOT_BYTES;
        memcpy(slot, src + off, len);
        HIPCHK(hipMemcpyAsync(dst + off, slot, len, hipMemcpyHostToDevice, st));
        if (record) HIPCHK(hipEventRecord(k->ev_slot[s], st));
        k->slot_used[s] = record;
    }
    return BK_OK;
}

// one row (or noise vector) to the device: a pageable one through the ring,
// a pinned or a device one by a copy of its own
int copy_row(Collect *k, void *dst, const void *src, size_t bytes, int where, hipStream_t st,
             bool record = true) {
    if (where == BK_HOST)
        return upload_pageable(k, (char *)dst, (const char *)src, bytes, st, record);
    HIPCHK(hipMemcpyAsync(dst, src, bytes,
                          where == BK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    return BK_OK;
}

// a call that added cnt rows succeeded: nothing is left to drain, the caller
// learns the first new slot and the rows count
int rows_added(Collect *k, Drain &drain, int64_t cnt, int64_t *first_slot) {
    drain.armed = false;
    if (first_slot && cnt > 0) *first_slot = k->count;
    k->count += cnt;
    return BK_OK;
}

// bk_collect_finish's arguments behind the context, as every finish takes them
struct FinishArgs {
    const int64_t *order;
    int64_t n, f;
    int64_t *sel_idx, *m_out;
    double *scores, *mean_out;
};

int finish_checked(bk_ctx *c, Collect *k, const FinishArgs &a);

// every order entry a collected slot (0..count-1), none repeated within its
// problem; slots may be reused across problems: seen[o] = 1 + the last problem
// b that used slot o (count zeros at the call's first problem).  b < 0: the
// single finish, whose messages carry no problem
int check_order(const int64_t *order, int64_t n, int64_t count, std::vector<int64_t> &seen,
                int64_t b) {
    // (formatted on the refusal only: a batch of 256 checks 256 orders per call)
    const auto who = [b] { return b < 0 ? std::string() : "problem " + std::to_string(b) + ": "; };
    const int64_t mark = b < 0 ? 1 : b + 1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o = order[i];
        if (o < 0 || o >= count)
            return fail(BK_EINVAL, "%sorder[%lld] = %lld is no collected slot (0..%lld)",
                        who().c_str(), (long long)i, (long long)o, (long long)count - 1);
        if (seen[(size_t)o] == mark)
            return fail(BK_EINVAL, "%sorder[%lld] = %lld repeats a slot", who().c_str(),
                        (long long)i, (long long)o);
        seen[(size_t)o] = mark;
    }
    return BK_OK;
}

// ---- the entries' checks, one per message.  `who` is the entry the message
// names: a fused entry answers as the add and the finish it stands for

int check_where(int where) {
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where %d", where);
    return BK_OK;
}

// the context's collection if one was begun, else null with BK_EINVAL's message
// set (the context mutex held, as for every check below that takes k)
Collect *begun(bk_ctx *c, const char *who) {
    Collect *k = c->collect;
    if (k && k->begun) return k;
    (void)fail(BK_EINVAL, "%s without bk_collect_begin", who);
    return nullptr;
}

int check_room(const Collect *k, const char *who, int64_t count) {
    if (count > k->n_cap - k->count)
        return fail(BK_EINVAL, "%s: %lld rows past n_cap=%lld (%lld collected)", who,
                    (long long)count, (long long)k->n_cap, (long long)k->count);
    return BK_OK;
}

int check_f64(const Collect *k, const char *who, const char *only) {
    if (k->dtype != BK_F64)
        return fail(BK_EINVAL, "%s: the collection is BK_F32 (%s)", who, only);
    return BK_OK;
}

// bk_collect_add_noised's checks that need no collection: k, noises and where
int check_noised_args(const double *const *noises, int64_t kn, int where) {
    if (kn < 0) return fail(BK_EINVAL, "need k >= 0 (k=%lld)", (long long)kn);
    if (!noises && kn > 0) return fail(BK_EINVAL, "null noises with k=%lld", (long long)kn);
    CHK(check_where(where));
    if (kn > BK_COLLECT_NOISE_MAX_K)
        return fail(BK_ENOTSUP, "k=%lld exceeds BK_COLLECT_NOISE_MAX_K=%d", (long long)kn,
                    BK_COLLECT_NOISE_MAX_K);
    return BK_OK;
}

// and those on the collection and on its count updates' pointers
int check_noised_updates(const Collect *k, const double *const *deltas,
                         const double *const *noises, int64_t kn, int64_t count) {
    CHK(check_f64(k, "bk_collect_add_noised", "noise is fp64 only"));
    CHK(check_room(k, "bk_collect_add_noised", count));
    for (int64_t i = 0; i < count; ++i) {
        if (!deltas[i]) return fail(BK_EINVAL, "null delta %lld", (long long)i);
        for (int64_t j = 0; j < kn; ++j)
            if (!noises[i * kn + j])
                return fail(BK_EINVAL, "null noise vector (%lld, %lld)", (long long)i, (long long)j);
    }
    return BK_OK;
}

// bk_collect_finish's checks against `rows` collected rows: the count, or
// count + 1 for the fused entries, whose row arrives in the same call
int check_finish(const Collect *k, int64_t rows, const int64_t *order, int64_t n, int64_t f) {
    if (n < 1 || n > rows)
        return fail(BK_EINVAL, "bk_collect_finish: n=%lld, %lld rows collected", (long long)n,
                    (long long)rows);
    if (!order && n != rows)
        return fail(BK_EINVAL, "bk_collect_finish: a null order needs n = %lld, the rows "
                               "collected (n=%lld)",
                    (long long)rows, (long long)n);
    CHK(bk_check_args(n, k->d, f));
    if (order) {
        std::vector<int64_t> seen((size_t)rows, 0);
        CHK(check_order(order, n, rows, seen, -1));
    }
    return BK_OK;
}

// The finish of n <= 128 rows in one launch: k_collect_small for the deployed
// shapes (small_ok: d <= 32,768; launch_collect_small) or, in the wide range
// (wide_ok), k_collect_wide, whose M items stream COLLECT_WIDE_COLS columns of
// the selected rows each (launch_collect_wide).  The kernel reads the Gram and
// the row store through the order in its own arguments and writes {margin,
// sel, scores, mean} into the context's mapped output block, so nothing is
// uploaded before it and nothing copied after it -- one launch, one wait, then
// host memcpys.  bk_collect_add_finish's fused launch (k_collect_arrive) goes
// the same way behind the new row's copy.  `launch` takes launch_collect_small's
// arguments; stat: the launch's counter in bk_collect_stats.  The arguments are
// validated by the caller.
template <typename L>
int finish_one_launch(bk_ctx *c, Collect *k, L launch, int stat, const FinishArgs &a) {
    static_assert(BK_MAX_N <= 65536, "arrival slots travel as 16-bit kernel arguments");
    const int64_t n = a.n, f = a.f, m = n - f, d = k->d;
    double *const scores = a.scores, *const mean_out = a.mean_out;
    constexpr size_t MPAD = HOUT_MPAD;
    CHK(ensure_small_queue(c));
    CHK(ensure(c->diag, (size_t)n * sizeof(double)));
    CHK(ensure_hout(c, MPAD + 2 * (size_t)n + (mean_out ? (size_t)d : 0)));
    double *blk = c->hout_dev;
    const uint64_t spin = next_spin(c);
    CHK(timed(c, BK_K_SMALL, [&] {
        return launch(k->store.p, k->dtype, k->ld, (int)n, d, (int)f, (const double *)k->G.p, a.order,
                      (double *)k->scores.p, (double *)c->diag.p, (int64_t *)(blk + MPAD),
                      mean_out ? blk + MPAD + 2 * n : nullptr, blk,
                      scores ? blk + MPAD + n : nullptr, (unsigned *)c->small_ctr.p, c->num_cu,
                      c->stream, spin, c->small_check_lines);
    }));
    ++k->stats[stat];
    c->margin_valid = 1;
    c->margin_host = c->hout_host_margin;
    c->margin_unchecked = 1;
    HIPCHK(wait_stream(c));
    const double *h = (const double *)c->hout;
    c->margin_unchecked = 0;
    CHK(margin_status(h));
    memcpy(a.sel_idx, h + MPAD, (size_t)m * sizeof(int64_t));
    if (scores) memcpy(scores, h + MPAD + n, (size_t)n * sizeof(double));
    if (mean_out) memcpy(mean_out, h + MPAD + 2 * n, (size_t)d * sizeof(double));
    if (a.m_out) *a.m_out = m;
    return BK_OK;
}

// The wide one-launch range (bk_set_collect_wide, off by default): n <= 128 and
// d past k_collect_small's cap.  The lower edge is the cap itself, not
// small_ok's (BK_SMALL_MAX_D may lower that one for A/Bs).  The upper edge
// depends on the mean: without one the launch does not depend on d and runs up
// to BK_COLLECT_WIDE_MAX_D; with one it stops at BK_COLLECT_WIDE_MEAN_MAX_D,
// past which the mean's way through the mapped block (written over PCIe by the
// kernel, then copied by the host) was measured behind the chain's DMA copy
// 
bool wide_ok(const bk_ctx *c, int64_t n, int64_t d, bool mean) {
    return c->small_on && c->collect_wide && n <= 128 && d > 32768 &&
           d <= (mean ? BK_COLLECT_WIDE_MEAN_MAX_D : BK_COLLECT_WIDE_MAX_D);
}

// the mean bytes one wide batched launch may write: BK_COLLECT_WIDE_OUT_BYTES,
// read at the call; it may only lower the default (1 GiB)
size_t wide_out_bytes() {
    const size_t dflt = (size_t)1 << 30;
    const char *e = getenv("BK_COLLECT_WIDE_OUT_BYTES");
    if (!e) return dflt;
    const long long v = atoll(e);
    return v > 0 && (size_t)v < dflt ? (size_t)v : dflt;
}

// the noise bytes one k_collect_noise launch may stage on the device:
// BK_COLLECT_NOISE_STAGE_BYTES, read at the call; it may only lower the
// default (256 MiB)
size_t noise_stage_bytes() {
    const size_t dflt = (size_t)256 << 20;
    const char *e = getenv("BK_COLLECT_NOISE_STAGE_BYTES");
    if (!e) return dflt;
    const long long v = atoll(e);
    return v > 0 && (size_t)v < dflt ? (size_t)v : dflt;
}

// ---- bk_set_collect_tiny: the one-workgroup collection (bk_collect_tiny.hip)

// The fused arrivals of the tiny range whose rows are longer than this take
// today's fused launches (k_collect_arrive, k_collect_arrive_noised) instead:
// bk_collect_add_finish from any source, and bk_collect_add_noised_finish from
// device rows.  At 16 x 128 fp64 (1 KiB rows) the three runs of the tiny call
// were not all below today's there (31.3 [27.3 .. 32.6] against 33.6 [30.1 ..
// 33.8] us plain; device rows 30.0 [25.3 .. 30.4] against 32.9 [30.1 .. 33.1] us
// with k = 1), at 200 B (10 x 25, 4 x 25) they were; nothing was measured in
// between.  Adds, finishes and the noised arrivals from host rows
// were ahead at every shape measured and stay
constexpr size_t TINY_ARRIVE_MAX_BYTES = 512;
bool tiny_arrive_ok(const Collect *k, bool cut) {
    return !cut || (size_t)k->d * esize(k->dtype) <= TINY_ARRIVE_MAX_BYTES;
}

constexpr size_t TINY_SLOT_STRIDE = (size_t)(1 + BK_COLLECT_NOISE_MAX_K) * COLLECT_TINY_SLOT_BYTES;

// The tiny range: the switch and the small path on, d <= 128 and at most 16
// rows collected after the call (a finish names collected slots only, so its n
// is in the range with them)
bool tiny_ok(const bk_ctx *c, const Collect *k, int64_t after) {
    return c->collect_tiny && after <= COLLECT_TINY_MAX_N && k->d <= COLLECT_TINY_MAX_D &&
           small_ok(c, k->store.p, k->dtype, after, k->d, k->ld);
}

// the arrival block, allocated whole at the first tiny call of the context's
// collection and kept: uncached on the device's side, so every load of a slot
// crosses PCIe and sees what the CPU wrote before the launch
int tiny_block(Collect *k) {
    if (k->arrive) return BK_OK;
    void *hp = nullptr, *dp = nullptr;
    const size_t bytes = (size_t)COLLECT_TINY_MAX_N * TINY_SLOT_STRIDE;
    hipError_t e = hipHostMalloc(&hp, bytes,
                                 hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess)
        return fail(BK_ENOMEM, "bk_collect: hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    e = hipHostGetDevicePointer(&dp, hp, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(hp);
        return fail(BK_EHIP, "bk_collect: hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    k->arrive = (char *)hp;
    k->arrive_dev = (char *)dp;
    return BK_OK;
}

// One call of the tiny range past its checks (the context mutex held, the
// device selected): cnt >= 0 rows arrive (kn > 0: as deltas with kn noise
// vectors each) and, with fz, the finish follows in the same launch.  Host rows
// are memcpy'd into their arrival slots, device rows are named in the launch
// arguments; no copy call anywhere.  A plain add is one launch for all its
// rows, a noised add one launch per row (the k pointers of one row fill the
// arguments), the finish rides on the last.  An add without a finish returns
// behind the launch -- host rows were consumed by the memcpy; device rows are
// waited for, as add_rows waits for their copies.  The rows count only when
// every launch was queued and, with a finish, completed (add_finish_fused's rule)
int tiny_call(bk_ctx *c, Collect *k, const void *const *rows, int64_t cnt,
              const double *const *noises, int64_t kn, int where, const FinishArgs *fz,
              int64_t *first_slot) {
    const hipStream_t st = c->stream;
    CHK(tiny_block(k));
    Drain drain{st};
    const size_t bytes = (size_t)k->d * esize(k->dtype);
    const int64_t j0 = k->count;
    const bool dev = where == BK_DEVICE;
    const int64_t per = kn > 0 || cnt == 0 ? 1 : cnt;  // rows per launch
    for (int64_t r0 = 0; r0 < (cnt > 0 ? cnt : 1); r0 += per) {
        const int64_t nr = cnt > 0 ? per : 0;
        const bool last = r0 + per >= cnt;
        CollectTinyLaunch L;
        L.store = k->store.p;
        L.dtype = k->dtype;
        L.ld = k->ld;
        L.d = k->d;
        L.G = (double *)k->G.p;
        L.j0 = (int)(j0 + r0);
        L.cnt = (int)nr;
        const double *vecs[BK_COLLECT_NOISE_MAX_K];
        for (int64_t r = 0; r < nr; ++r) {
            const size_t at = (size_t)(j0 + r0 + r) * TINY_SLOT_STRIDE;
            if (dev) {
                L.src[r] = rows[r0 + r];
            } else {
                memcpy(k->arrive + at, rows[r0 + r], bytes);
                L.src[r] = k->arrive_dev + at;
            }
            for (int64_t q = 0; q < kn; ++q) {  // (kn > 0: nr = 1)
                const size_t vat = at + (size_t)(1 + q) * COLLECT_TINY_SLOT_BYTES;
                if (dev) {
                    vecs[q] = noises[(r0 + r) * kn + q];
                } else {
                    memcpy(k->arrive + vat, noises[(r0 + r) * kn + q], bytes);
                    vecs[q] = (const double *)(k->arrive_dev + vat);
                }
            }
        }
        L.vecs = vecs;
        L.k = (int)kn;
        if (fz && last) {
            const auto launch = [&](const void *, int, int64_t, int n_, int64_t, int f_, const double *,
                                    const int64_t *ord, double *, double *, int64_t *sel,
                                    double *mean, double *margin, double *sc_out, unsigned *, int,
                                    hipStream_t s, uint64_t, int) {
                L.fin = 1;
                L.n = n_;
                L.f = f_;
                L.order = ord;
                L.sel = sel;
                L.mean = mean;
                L.margin = margin;
                L.scores_out = sc_out;
                return launch_collect_tiny(L, s);
            };
            CHK(finish_one_launch(c, k, launch, nr > 0 ? 3 : 2, *fz));
            ++k->tiny_stats[nr > 0 ? 2 : 1];
        } else {
            CHK(timed(c, BK_K_SMALL, [&] { return launch_collect_tiny(L, st); }));
            ++k->tiny_stats[0];
        }
    }
    // device rows are read by the kernel itself: consumed once it is done
    if (dev && cnt > 0 && !fz) HIPCHK(hipStreamSynchronize(st));
    return rows_added(k, drain, cnt, first_slot);
}

// bk_collect_add past its checks (the context mutex held): the rows copied into
// the slots from count on, then their border
int add_rows(bk_ctx *c, Collect *k, const void *const *rows, int64_t count, int where,
             int64_t *first_slot) {
    DeviceGuard dg(c->device);
    if (tiny_ok(c, k, k->count + count))
        return tiny_call(c, k, rows, count, nullptr, 0, where, nullptr, first_slot);
    const hipStream_t st = c->stream;
    Drain drain{st};
    const size_t es = esize(k->dtype), bytes = (size_t)k->d * es;
    const int64_t j0 = k->count;
    for (int64_t i = 0; i < count; ++i)
        CHK(copy_row(k, (char *)k->store.p + (size_t)(j0 + i) * (size_t)k->ld * es, rows[i], bytes,
                     where, st));
    if (where != BK_HOST) HIPCHK(hipEventRecord(k->ev_up, st));
    CHK(fold_border(k, j0, count, c->num_cu, st));
    // pinned and device rows are read by the copies themselves: consumed once
    // those are done (the border runs on)
    if (where != BK_HOST) HIPCHK(hipEventSynchronize(k->ev_up));
    return rows_added(k, drain, count, first_slot);
}

// bk_collect_add_finish's fused path past its checks (the context mutex held,
// the device selected; count + 1 <= 128 and the finish small_ok): the row goes
// to slot `count` as add_rows copies it, then ONE launch -- k_collect_arrive,
// the border of that slot in front of k_collect_small's items -- and the one
// wait of finish_one_launch, behind which the row has been consumed.  The
// collection counts the row only when all of it succeeded: after a failure the
// next add rewrites the slot and its Gram run.  wide (bk_set_collect_wide_arrive;
// a pinned or a device row, the finish wide_ok): the launch is
// k_collect_arrive_wide, whose border partials meet in the collection's P
int add_finish_fused(bk_ctx *c, Collect *k, const void *row, int where, int64_t *first_slot,
                     const FinishArgs &a, bool wide = false) {
    const hipStream_t st = c->stream;
    Drain drain{st};
    const size_t es = esize(k->dtype), bytes = (size_t)k->d * es;
    const int64_t j = k->count;
    // (a pageable row of the fused range is one ring slot: d <= 32,768; the
    // stream is waited for below, or drained on a failure, before any later add)
    CHK(copy_row(k, (char *)k->store.p + (size_t)j * (size_t)k->ld * es, row, bytes, where, st,
                 false));
    double *const P = (double *)k->P.p;
    const auto launch = [j, wide, P](const void *store, int dtype, int64_t ld, int n_, int64_t d,
                                     int f_, const double *G, const int64_t *ord, double *sc,
                                     double *diag, int64_t *sel, double *mean, double *margin,
                                     double *sc_out, unsigned *ctr, int num_cu, hipStream_t s,
                                     uint64_t spin, int lines) {
        if (wide)
            return launch_collect_arrive_wide(store, dtype, ld, (int)j, n_, d, f_,
                                              const_cast<double *>(G), P, ord, sc, diag, sel, mean,
                                              margin, sc_out, ctr, num_cu, s, spin, lines);
        return launch_collect_arrive(store, dtype, ld, (int)j, n_, d, f_, const_cast<double *>(G),
                                     ord, sc, diag, sel, mean, margin, sc_out, ctr, num_cu, s, spin,
                                     lines);
    };
    CHK(finish_one_launch(c, k, launch, 3, a));
    return rows_added(k, drain, 1, first_slot);
}

// bk_collect_add_noised past its checks, k >= 1 (fp64 collection, the context
// mutex held).  Host rows: every delta goes to its store row as add_rows
// uploads it, the noise vectors of a launch to the staging block, and
// k_collect_noise adds them in place.  Device rows: the kernel reads the
// caller's deltas and, through one uploaded pointer table, its noise vectors
// where they are.  A launch covers up to BORDER_ROWS rows, as many as the
// staging bound holds; a row whose k vectors exceed it is noised in consecutive
// ranges of an even number of columns (every element is independent: the same
// bits however the call is cut).  Then the border of the new slots
int add_noised(bk_ctx *c, Collect *k, const double *const *deltas, const double *const *noises,
               int64_t kn, int64_t count, int where, int64_t *first_slot) {
    static_assert(COLLECT_NOISE_ROWS == BORDER_ROWS, "one noise launch per border group");
    DeviceGuard dg(c->device);
    if (tiny_ok(c, k, k->count + count))
        return tiny_call(c, k, (const void *const *)deltas, count, noises, kn, where, nullptr,
                         first_slot);
    const hipStream_t st = c->stream;
    const int64_t j0 = k->count, d = k->d;
    const size_t bytes = (size_t)d * sizeof(double);
    const bool dev = where == BK_DEVICE;
    // rows per launch and columns per range
    int64_t fit = BORDER_ROWS, wcols = d;
    if (dev) {
        const size_t tb = (size_t)count * (size_t)kn * sizeof(double *);
        // (a launch of an earlier add may still read the block about to be replaced)
        if (tb > k->ntab.bytes) HIPCHK(hipStreamSynchronize(st));
        CHK(grow_all({{&k->ntab, tb}, {&k->hntab, tb}}, "bk_collect_add_noised"));
    } else {
        const size_t bound = noise_stage_bytes();
        const size_t row = (size_t)kn * (size_t)((d + 1) & ~(int64_t)1) * sizeof(double);
        if (row <= bound) {
            fit = (int64_t)(bound / row) < fit ? (int64_t)(bound / row) : fit;
            if (fit > count) fit = count;
        } else {
            fit = 1;
            wcols = (int64_t)(bound / ((size_t)kn * sizeof(double))) & ~(int64_t)1;
            if (wcols < 2) wcols = 2;
        }
        const size_t need = (size_t)fit * (size_t)kn * (size_t)((wcols + 1) & ~(int64_t)1) * sizeof(double);
        if (need > k->nstage.bytes) HIPCHK(hipStreamSynchronize(st));
        CHK(grow_all({{&k->nstage, need}}, "bk_collect_add_noised"));
    }
    Drain drain{st};
    double *store = (double *)k->store.p;
    if (dev) {
        const double **ht = (const double **)k->hntab.p;
        for (int64_t q = 0; q < count * kn; ++q) ht[q] = noises[q];
        HIPCHK(hipMemcpyAsync(k->ntab.p, ht, (size_t)count * (size_t)kn * sizeof(double *),
                              hipMemcpyHostToDevice, st));
    } else {
        for (int64_t i = 0; i < count; ++i)
            CHK(copy_row(k, store + (j0 + i) * k->ld, deltas[i], bytes, where, st));
    }
    for (int64_t r0 = 0; r0 < count; r0 += fit) {
        const int nr = (int)(count - r0 < fit ? count - r0 : fit);
        for (int64_t c0 = 0; c0 < d; c0 += wcols) {
            const int64_t c1 = c0 + wcols < d ? c0 + wcols : d;
            CollectNoiseArgs a = {};
            a.sld = (c1 - c0 + 1) & ~(int64_t)1;
            a.c0 = c0;
            a.c1 = c1;
            a.rows = nr;
            a.k = (int)kn;
            if (dev)
                a.tab = (const double *const *)k->ntab.p + r0 * kn;
            else
                a.stage = (const double *)k->nstage.p;
            for (int r = 0; r < nr; ++r) {
                a.out[r] = store + (j0 + r0 + r) * k->ld;
                a.delta[r] = dev ? deltas[r0 + r] : a.out[r];
                for (int64_t j = 0; j < kn && !dev; ++j)
                    CHK(copy_row(k, (double *)k->nstage.p + (r * kn + j) * a.sld,
                                 noises[(r0 + r) * kn + j] + c0, (size_t)(c1 - c0) * sizeof(double),
                                 where, st));
            }
            // pinned rows are read by the copies: consumed with the last of them
            if (where == BK_HOST_PINNED && r0 + nr == count && c1 == d)
                HIPCHK(hipEventRecord(k->ev_up, st));
            CHK(timed(c, BK_K_NOISE, [&] { return launch_collect_noise(a, c->num_cu, st); }));
        }
    }
    // device rows are read by the kernel itself: consumed with the last launch
    if (dev) HIPCHK(hipEventRecord(k->ev_up, st));
    CHK(fold_border(k, j0, count, c->num_cu, st));
    if (where != BK_HOST) HIPCHK(hipEventSynchronize(k->ev_up));  // (the border runs on)
    return rows_added(k, drain, count, first_slot);
}

// bk_collect_add_finish past its checks (the context mutex held, the device
// selected)
int add_finish_checked(bk_ctx *c, Collect *k, const void *row, int where, int64_t *first_slot,
                       const FinishArgs &a) {
    if (tiny_ok(c, k, k->count + 1) && tiny_arrive_ok(k, true))
        return tiny_call(c, k, &row, 1, nullptr, 0, where, &a, first_slot);
    // the fused launch: the finish in k_collect_small's range, a border of at
    // most 128 rows and no long pageable row; everything else is the two
    // entries' own paths
    const bool long_host = where == BK_HOST && (size_t)k->d * esize(k->dtype) > ARRIVE_HOST_MAX_BYTES;
    if (k->count + 1 <= 128 && !long_host && small_ok(c, k->store.p, k->dtype, a.n, k->d, k->ld))
        return add_finish_fused(c, k, row, where, first_slot, a);
    // the fused wide launch (bk_set_collect_wide_arrive): the finish in
    // k_collect_wide's range, a border of at most 128 rows, a pinned or a device
    // row (a pageable row this long is past ARRIVE_HOST_MAX_BYTES); with on = 1
    // only where it was measured ahead (ARRIVE_WIDE_MAX_BYTES)
    const bool wide_cut = c->collect_wide_arrive == 1 &&
                          !(where == BK_HOST_PINNED && a.mean_out &&
                            (size_t)k->d * esize(k->dtype) <= ARRIVE_WIDE_MAX_BYTES);
    if (c->collect_wide_arrive && !wide_cut && k->count + 1 <= 128 && where != BK_HOST &&
        wide_ok(c, a.n, k->d, a.mean_out != nullptr))
        return add_finish_fused(c, k, row, where, first_slot, a, true);
    CHK(add_rows(c, k, &row, 1, where, first_slot));
    return finish_checked(c, k, a);
}

// bk_collect_add_noised_finish's fused path past its checks, k >= 1 (fp64
// collection, the context mutex held, the device selected; count + 1 <= 128 and
// the finish small_ok).  Host rows: the delta goes to slot `count` as add_rows
// copies it and the k noise vectors to the staging block; device rows are read
// where they are and nothing is copied.  Then ONE launch -- k_collect_arrive_noised:
// the noise of that slot, its border and k_collect_small's items -- and the one
// wait of finish_one_launch, behind which every input has been consumed.  The
// k vectors' pointers travel in the launch arguments: no table upload.  The
// collection counts the row only when all of it succeeded (add_finish_fused)
int add_noised_finish_fused(bk_ctx *c, Collect *k, const double *delta,
                            const double *const *noises, int64_t kn, int where,
                            int64_t *first_slot, const FinishArgs &a) {
    static_assert(BK_COLLECT_NOISE_MAX_K == COLLECT_ARRIVE_NOISE_MAX_K, "the launch's vector table");
    const hipStream_t st = c->stream;
    const int64_t j = k->count, d = k->d;
    const size_t bytes = (size_t)d * sizeof(double);
    const int64_t sld = (d + 1) & ~(int64_t)1;
    const bool dev = where == BK_DEVICE;
    if (!dev) {
        const size_t need = (size_t)kn * (size_t)sld * sizeof(double);
        // (a launch of an earlier add may still read the block about to be replaced)
        if (need > k->nstage.bytes) HIPCHK(hipStreamSynchronize(st));
        CHK(grow_all({{&k->nstage, need}}, "bk_collect_add_noised"));
    }
    Drain drain{st};
    double *rowj = (double *)k->store.p + j * k->ld;
    const double *vecs[BK_COLLECT_NOISE_MAX_K];
    // (a row of the fused range is one ring slot: d <= 32,768.  The stream is
    // waited for below, or drained on a failure, before any later add; up to
    // RING_SLOTS copies need no event behind them, more of them reuse a slot
    // within the call and take upload_pageable's events)
    const bool record = 1 + kn > RING_SLOTS;
    if (dev) {
        for (int64_t q = 0; q < kn; ++q) vecs[q] = noises[q];
    } else {
        CHK(copy_row(k, rowj, delta, bytes, where, st, record));
        for (int64_t q = 0; q < kn; ++q) {
            double *dst = (double *)k->nstage.p + q * sld;
            CHK(copy_row(k, dst, noises[q], bytes, where, st, record));
            vecs[q] = dst;
        }
    }
    const double *dsrc = dev ? delta : rowj;
    const auto launch = [&](const void *store, int, int64_t ld, int n_, int64_t d_, int f_,
                            const double *G, const int64_t *ord, double *sc, double *diag,
                            int64_t *sel, double *mean, double *margin, double *sc_out,
                            unsigned *ctr, int num_cu, hipStream_t s, uint64_t spin, int lines) {
        return launch_collect_arrive_noised(store, ld, (int)j, dsrc, vecs, (int)kn, n_, d_, f_,
                                            const_cast<double *>(G), ord, sc, diag, sel, mean,
                                            margin, sc_out, ctr, num_cu, s, spin, lines);
    };
    CHK(finish_one_launch(c, k, launch, 3, a));
    return rows_added(k, drain, 1, first_slot);
}

}  // namespace

extern "C" {

int bk_collect_begin(bk_ctx *c, int dtype, int64_t n_cap, int64_t d) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype %d", dtype);
    if (n_cap < 1 || d < 1)
        return fail(BK_EINVAL, "need n_cap >= 1 and d >= 1 (n_cap=%lld d=%lld)", (long long)n_cap,
                    (long long)d);
    if (n_cap > BK_MAX_N)
        return fail(BK_EINVAL, "n_cap=%lld exceeds BK_MAX_N=%d", (long long)n_cap, BK_MAX_N);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    const hipStream_t st = c->stream;
    Collect *k = c->collect;
    if (!k) {
        k = new (std::nothrow) Collect();
        if (!k) return fail(BK_ENOMEM, "host allocation of the collection failed");
        k->horder.pinned = k->ring.pinned = k->b_horder.pinned = k->hntab.pinned = true;
        hipError_t e = hipEventCreateWithFlags(&k->ev_up, hipEventDisableTiming);
        for (int s = 0; s < RING_SLOTS && e == hipSuccess; ++s)
            e = hipEventCreateWithFlags(&k->ev_slot[s], hipEventDisableTiming);
        if (e != hipSuccess) {
            collect_destroy(k);
            return fail(BK_EHIP, "bk_collect_begin: events: %s", hipGetErrorString(e));
        }
        c->collect = k;
    }
    const size_t es = esize(dtype);
    const int64_t per16 = 16 / (int64_t)es;
    const int64_t ld = (d + per16 - 1) / per16 * per16;
    const int S = (int)(((size_t)d * es + BORDER_CHUNK_BYTES - 1) / BORDER_CHUNK_BYTES);
    const int64_t m_max = n_cap;
    const size_t un = (size_t)n_cap;
    // work of the old collection may still read the buffers about to be replaced
    HIPCHK(hipStreamSynchronize(st));
    // a collection that regrows lets go of the batched finish's buffers
    if (un * (size_t)ld * es > k->store.bytes || un * (un + 1) / 2 * sizeof(double) > k->G.bytes)
        collect_batch_release(k);
    CHK(grow_all({{&k->store, un * (size_t)ld * es},
                  {&k->G, un * (un + 1) / 2 * sizeof(double)},
                  {&k->P, (size_t)S * BORDER_ROWS * un * sizeof(double)},
                  {&k->U, (size_t)bk_upper_elems(n_cap) * sizeof(double)},
                  {&k->sel, un * sizeof(int64_t)},
                  {&k->slots, un * sizeof(int64_t)},
                  {&k->scores, un * sizeof(double)},
                  {&k->mean, (size_t)d * sizeof(double)},
                  {&k->mean_part, mean_segments((int)m_max) > 1
                                      ? (size_t)mean_segments((int)m_max) * (size_t)d * sizeof(double)
                                      : 0},
                  {&k->order, un * sizeof(int64_t)},
                  {&k->horder, un * sizeof(int64_t)},
                  {&k->ring, RING_SLOT_BYTES * RING_SLOTS}}));
    // the rows' pad columns [d, ld) are read by k_border's 16-B loads: zero
    if (ld > d) {
        const hipError_t e =
            hipMemset2DAsync((char *)k->store.p + (size_t)d * es, (size_t)ld * es, 0,
                             (size_t)(ld - d) * es, un, st);
        if (e != hipSuccess) {
            k->begun = false;  // the buffers were replaced: no collection
            k->count = 0;
            return fail(BK_EHIP, "bk_collect_begin: hipMemset2DAsync: %s", hipGetErrorString(e));
        }
    }
    k->begun = true;
    k->dtype = dtype;
    k->n_cap = n_cap;
    k->d = d;
    k->ld = ld;
    k->S = S;
    k->count = 0;
    for (int64_t &v : k->stats) v = 0;
    for (int64_t &v : k->tiny_stats) v = 0;
    return BK_OK;
}

int bk_collect_add(bk_ctx *c, const void *const *rows, int64_t count, int where,
                   int64_t *first_slot) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!rows) return fail(BK_EINVAL, "null rows");
    if (count < 1) return fail(BK_EINVAL, "need count >= 1 (count=%lld)", (long long)count);
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_add");
    if (!k) return BK_EINVAL;
    CHK(check_room(k, "bk_collect_add", count));
    for (int64_t i = 0; i < count; ++i)
        if (!rows[i]) return fail(BK_EINVAL, "null row %lld", (long long)i);
    return add_rows(c, k, rows, count, where, first_slot);
}

int bk_collect_add_noised(bk_ctx *c, const double *const *deltas, const double *const *noises,
                          int64_t kn, int64_t count, int where, int64_t *first_slot) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!deltas) return fail(BK_EINVAL, "null deltas");
    if (count < 1) return fail(BK_EINVAL, "need count >= 1 (count=%lld)", (long long)count);
    CHK(check_noised_args(noises, kn, where));
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_add_noised");
    if (!k) return BK_EINVAL;
    CHK(check_noised_updates(k, deltas, noises, kn, count));
    // no noisers: the row is the delta, bitwise (bk_multikrum_noised's rule)
    if (kn == 0)
        return add_rows(c, k, (const void *const *)deltas, count, where, first_slot);
    return add_noised(c, k, deltas, noises, kn, count, where, first_slot);
}

int bk_collect_read_rows(bk_ctx *c, const int64_t *slots, int64_t count, double *const *out_rows) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!slots) return fail(BK_EINVAL, "null slots");
    if (!out_rows) return fail(BK_EINVAL, "null out_rows");
    if (count < 1) return fail(BK_EINVAL, "need count >= 1 (count=%lld)", (long long)count);
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_read_rows");
    if (!k) return BK_EINVAL;
    CHK(check_f64(k, "bk_collect_read_rows", "fp64 rows only"));
    for (int64_t i = 0; i < count; ++i)
        if (slots[i] < 0 || slots[i] >= k->count)
            return fail(BK_EINVAL, "slots[%lld] = %lld is no collected slot (0..%lld)", (long long)i,
                        (long long)slots[i], (long long)k->count - 1);
    for (int64_t i = 0; i < count; ++i)
        if (!out_rows[i]) return fail(BK_EINVAL, "null output row %lld", (long long)i);
    DeviceGuard dg(c->device);
    const hipStream_t st = c->stream;
    Drain drain{st};
    for (int64_t i = 0; i < count; ++i)
        HIPCHK(hipMemcpyAsync(out_rows[i], (const double *)k->store.p + slots[i] * k->ld,
                              (size_t)k->d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    drain.armed = false;
    return BK_OK;
}

int bk_collect_count(bk_ctx *c, int64_t *count) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!count) return fail(BK_EINVAL, "null count");
    std::lock_guard<std::mutex> lk(c->mu);
    const Collect *k = c->collect;
    *count = k && k->begun ? k->count : 0;
    return BK_OK;
}

int bk_collect_finish(bk_ctx *c, const int64_t *order, int64_t n, int64_t f, int64_t *sel_idx,
                      int64_t *m_out, double *scores, double *mean_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_finish");
    if (!k) return BK_EINVAL;
    CHK(check_finish(k, k->count, order, n, f));
    DeviceGuard dg(c->device);
    return finish_checked(c, k, {order, n, f, sel_idx, m_out, scores, mean_out});
}

int bk_collect_add_finish(bk_ctx *c, const void *row, int where, const int64_t *order, int64_t n,
                          int64_t f, int64_t *first_slot, int64_t *sel_idx, int64_t *m_out,
                          double *scores, double *mean_out) {
    // bk_collect_add's checks, then bk_collect_finish's on count + 1 rows
    if (!c) return fail(BK_EINVAL, "null context");
    if (!row) return fail(BK_EINVAL, "null row 0");
    CHK(check_where(where));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_add");
    if (!k) return BK_EINVAL;
    CHK(check_room(k, "bk_collect_add", 1));
    CHK(check_finish(k, k->count + 1, order, n, f));
    DeviceGuard dg(c->device);
    return add_finish_checked(c, k, row, where, first_slot,
                              {order, n, f, sel_idx, m_out, scores, mean_out});
}

int bk_collect_add_noised_finish(bk_ctx *c, const double *delta, const double *const *noises,
                                 int64_t kn, int where, const int64_t *order, int64_t n, int64_t f,
                                 int64_t *first_slot, int64_t *sel_idx, int64_t *m_out,
                                 double *scores, double *mean_out) {
    // bk_collect_add_noised's checks on one update, then bk_collect_finish's on
    // count + 1 rows, as bk_collect_add_finish does them
    if (!c) return fail(BK_EINVAL, "null context");
    if (!delta) return fail(BK_EINVAL, "null delta 0");
    CHK(check_noised_args(noises, kn, where));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_add_noised");
    if (!k) return BK_EINVAL;
    CHK(check_noised_updates(k, &delta, noises, kn, 1));
    CHK(check_finish(k, k->count + 1, order, n, f));
    DeviceGuard dg(c->device);
    const FinishArgs a = {order, n, f, sel_idx, m_out, scores, mean_out};
    // no noisers: the row is the delta, bk_collect_add_finish's path and bits
    if (kn == 0) return add_finish_checked(c, k, delta, where, first_slot, a);
    if (tiny_ok(c, k, k->count + 1) && tiny_arrive_ok(k, where == BK_DEVICE))
        return tiny_call(c, k, (const void *const *)&delta, 1, noises, kn, where, &a, first_slot);
    // the fused launch: the finish in k_collect_small's range, a border of at
    // most 128 rows, and of the long host rows only pinned ones with one noise
    // vector (ARRIVE_NOISED_HOST_MAX_BYTES); everything else is the two
    // entries' own paths
    const bool long_host = where != BK_DEVICE && !(where == BK_HOST_PINNED && kn == 1) &&
                           (size_t)k->d * sizeof(double) > ARRIVE_NOISED_HOST_MAX_BYTES;
    if (k->count + 1 <= 128 && !long_host && small_ok(c, k->store.p, k->dtype, n, k->d, k->ld))
        return add_noised_finish_fused(c, k, delta, noises, kn, where, first_slot, a);
    CHK(add_noised(c, k, &delta, noises, kn, 1, where, first_slot));
    return finish_checked(c, k, a);
}

int bk_collect_stats(bk_ctx *c, int64_t out[4]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    const Collect *k = c->collect;
    for (int i = 0; i < 4; ++i) out[i] = k && k->begun ? k->stats[i] : 0;
    return BK_OK;
}

int bk_collect_tiny_stats(bk_ctx *c, int64_t out[3]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    const Collect *k = c->collect;
    for (int i = 0; i < 3; ++i) out[i] = k && k->begun ? k->tiny_stats[i] : 0;
    return BK_OK;
}

}  // extern "C"

namespace {

// bk_collect_finish past its checks (the context mutex held, the device selected)
int finish_checked(bk_ctx *c, Collect *k, const FinishArgs &a) {
    const auto [order, n, f, sel_idx, m_out, scores, mean_out] = a;
    if (tiny_ok(c, k, k->count)) return tiny_call(c, k, nullptr, 0, nullptr, 0, BK_HOST, &a, nullptr);
    if (small_ok(c, k->store.p, k->dtype, n, k->d, k->ld))
        return finish_one_launch(c, k, launch_collect_small, 2, a);
    if (wide_ok(c, n, k->d, mean_out != nullptr))
        return finish_one_launch(c, k, launch_collect_wide, 2, a);
    const hipStream_t st = c->stream;
    Drain drain{st};
    int64_t *ho = (int64_t *)k->horder.p;
    for (int64_t i = 0; i < n; ++i) ho[i] = order ? order[i] : i;
    int64_t *dord = (int64_t *)k->order.p, *dsel = (int64_t *)k->sel.p;
    double *U = (double *)k->U.p, *dsc = (double *)k->scores.p;
    const int64_t m = n - f;
    HIPCHK(hipMemcpyAsync(dord, ho, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const int T = (int)((n + 63) / 64);
    hipLaunchKernelGGL(k_collect_gather, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, st,
                       (const double *)k->G.p, (const int64_t *)dord, (int)n, T, (double)k->d, U);
    HIPCHK(hipGetLastError());
    // K2, K3, K3b and the margin record, unchanged, on the gathered record
    Plan pl;
    pl.n = (int)n;
    pl.T = (int)((n + 63) / 64);
    pl.ntile = pl.T * (pl.T + 1) / 2;
    CHK(stage_finish(c, U, pl, nullptr, BK_F64, n, 0, 0, f, dsel, dsc, nullptr));
    double *dmean = nullptr;
    if (mean_out) {
        dmean = (double *)k->mean.p;
        int64_t *slots = (int64_t *)k->slots.p;
        hipLaunchKernelGGL(k_collect_selmap, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st,
                           (const int64_t *)dsel, (const int64_t *)dord, (int)m, slots);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_mean(k->store.p, k->dtype, k->ld, k->d, slots, (int)m, dmean, c->num_cu, st,
                           mean_segments((int)m) > 1 ? (double *)k->mean_part.p : nullptr));
    }
    HIPCHK(hipMemcpyAsync(sel_idx, dsel, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (scores)
        HIPCHK(hipMemcpyAsync(scores, dsc, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (mean_out)
        HIPCHK(hipMemcpyAsync(mean_out, dmean, (size_t)k->d * sizeof(double), hipMemcpyDeviceToHost,
                              st));
    HIPCHK(wait_stream(c));
    CHK(check_margin_readback(c));
    drain.armed = false;
    if (m_out) *m_out = m;
    return BK_OK;
}

// What bk_collect_finish_batch's launches (finish_batch_small) and
// bk_collect_finish_ragged's (finish_ragged) share on the host: the buffers,
// the read-back and the closing bookkeeping.

// The collection's batch buffers for `batch` problems in launches of at most W:
// obytes of staged orders (device and pinned), nsc scores and diag, nsel
// selected indices, the means, the queue lines (zeroed when they grow; every
// launch leaves them zero) and the context's record store.  (Every user of
// these buffers is synchronous: none is in use when it grows)
int batch_buffers(bk_ctx *c, Collect *k, const char *who, int64_t batch, int64_t W, size_t obytes,
                  size_t nsc, size_t nsel, bool mean) {
    const size_t lbytes =
        (size_t)(COLLECT_BATCH_QLINES + W * COLLECT_BATCH_LINES) * 32 * sizeof(unsigned);
    const bool new_lines = lbytes > k->b_ctr.bytes;
    CHK(grow_all({{&k->b_order, obytes},
                  {&k->b_horder, obytes},
                  {&k->b_scores, nsc * sizeof(double)},
                  {&k->b_diag, nsc * sizeof(double)},
                  {&k->b_sel, nsel * sizeof(int64_t)},
                  {&k->b_mean, mean ? (size_t)batch * (size_t)k->d * sizeof(double) : 0},
                  {&k->b_ctr, lbytes}},
                 who));
    CHK(ensure(c->batch_rec, (size_t)batch * MARGIN_WORDS * sizeof(double)));
    if (new_lines) HIPCHK(hipMemsetAsync(k->b_ctr.p, 0, k->b_ctr.bytes, c->stream));
    return BK_OK;
}

// The records (to recs), sel, scores and the means come back whole after the
// last launch, under one timing bracket and the one wait
int batch_readback(bk_ctx *c, Collect *k, int64_t batch, size_t nsc, size_t nsel, double *recs,
                   int64_t *sel_idx, double *scores, double *mean_out) {
    const hipStream_t st = c->stream;
    const size_t ub = (size_t)batch;
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(recs, c->batch_rec.p, ub * MARGIN_WORDS * sizeof(double),
                                      hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(sel_idx, k->b_sel.p, nsel * sizeof(int64_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && scores)
            e = hipMemcpyAsync(scores, k->b_scores.p, nsc * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && mean_out)
            e = hipMemcpyAsync(mean_out, k->b_mean.p, ub * (size_t)k->d * sizeof(double),
                               hipMemcpyDeviceToHost, st);
        return e;
    }));
    HIPCHK(wait_stream(c));
    return BK_OK;
}

// The stream is idle and batch_rec_h holds the call's records: the context's
// record is the batch's pick, checked here (an error code wins the pick: a
// give-up marks every problem of its launch)
int batch_close(bk_ctx *c, int64_t batch) {
    c->batch_one = 0;
    c->batch_last = batch;
    batch_pick_record(c);
    c->margin_valid = 1;
    c->margin_host = c->batch_pick;
    c->margin_unchecked = 0;
    return margin_status(c->batch_pick);
}

// One problem of a batch by the single finish, which is synchronous and leaves
// its record in host memory: the record is copied behind it straight to rec,
// the problem's place in the host side of the batch record store -- no copy to
// the device and none back
int finish_one_of_batch(bk_ctx *c, Collect *k, const int64_t *order, int64_t n, int64_t f,
                        int64_t *sel_idx, double *scores, double *mean_out, double *rec) {
    CHK(finish_checked(c, k, {order, n, f, sel_idx, nullptr, scores, mean_out}));
    memcpy(rec, c->margin_host, MARGIN_WORDS * sizeof(double));
    return BK_OK;
}

// The batch within k_collect_small's range: launches of W <= SMALL_BATCH_MAX_W
// problems (k_collect_small_batch, bk_collect_batch.hip) on buffers of the
// collection's own; the slots go up as 16-bit numbers in one copy from pinned
// staging, the outputs come back after the last launch, then one wait.  The
// records land in the context's batch record store (bk_batch.hip batch_fetch).
int finish_batch_small(bk_ctx *c, Collect *k, const int64_t *orders, int64_t batch, int64_t n,
                       int64_t f, int64_t *sel_idx, double *scores, double *mean_out) {
    const int64_t m = n - f, d = k->d;
    const hipStream_t st = c->stream;
    const size_t ub = (size_t)batch, un = (size_t)n;
    const int64_t W = batch < SMALL_BATCH_MAX_W ? batch : SMALL_BATCH_MAX_W;
    CHK(batch_buffers(c, k, "bk_collect_finish_batch", batch, W, ub * un * sizeof(uint16_t), ub * un,
                      ub * (size_t)m, mean_out != nullptr));
    Drain drain{st};
    uint16_t *ho = (uint16_t *)k->b_horder.p;
    for (size_t i = 0; i < ub * un; ++i) ho[i] = (uint16_t)orders[i];  // validated: < count <= 65,536
    CHK(timed(c, BK_K_H2D, [&] {
        return hipMemcpyAsync(k->b_order.p, ho, ub * un * sizeof(uint16_t), hipMemcpyHostToDevice, st);
    }));
    double *dsc = (double *)k->b_scores.p, *ddg = (double *)k->b_diag.p;
    double *dmean = mean_out ? (double *)k->b_mean.p : nullptr;
    int64_t *dsel = (int64_t *)k->b_sel.p;
    for (int64_t b0 = 0; b0 < batch; b0 += W) {
        const int w = (int)(batch - b0 < W ? batch - b0 : W);
        const uint64_t spin = next_spin(c);
        CHK(timed(c, BK_K_SMALL, [&] {
            return launch_collect_small_batch(
                k->store.p, k->dtype, k->ld, w, (int)n, d, (int)f, (const double *)k->G.p,
                (const uint16_t *)k->b_order.p + b0 * n, dsc + b0 * n, ddg + b0 * n, dsel + b0 * m,
                dmean ? dmean + b0 * d : nullptr, (double *)c->batch_rec.p + b0 * MARGIN_WORDS,
                (unsigned *)k->b_ctr.p, c->num_cu, st, spin);
        }));
    }
    // the launches are queued: from here the context's record is this batch's,
    // unchecked until the wait is over (batch_close states the rest again)
    c->batch_one = 0;
    c->margin_valid = 1;
    c->margin_host = c->batch_pick;
    c->margin_unchecked = 1;
    c->batch_last = batch;
    c->batch_fetched = 0;
    // the records come back with the outputs, under the same wait
    c->batch_rec_h.resize(ub * MARGIN_WORDS);
    CHK(batch_readback(c, k, batch, ub * un, ub * (size_t)m, c->batch_rec_h.data(), sel_idx, scores,
                       mean_out));
    drain.armed = false;
    return batch_close(c, batch);
}

// Outside that range, and for one problem: the single finish per problem
int finish_batch_loop(bk_ctx *c, Collect *k, const int64_t *orders, int64_t batch, int64_t n,
                      int64_t f, int64_t *sel_idx, double *scores, double *mean_out) {
    const int64_t m = n - f;
    std::vector<double> recs((size_t)batch * MARGIN_WORDS);
    for (int64_t b = 0; b < batch; ++b)
        CHK(finish_one_of_batch(c, k, orders + b * n, n, f, sel_idx + b * m,
                                scores ? scores + b * n : nullptr,
                                mean_out ? mean_out + b * k->d : nullptr,
                                recs.data() + (size_t)b * MARGIN_WORDS));
    c->batch_rec_h.swap(recs);
    return batch_close(c, batch);  // (every finish checked its own record)
}

int finish_ragged(bk_ctx *c, Collect *k, const int64_t *orders, const int64_t *offsets,
                  const int64_t *fs, int64_t batch, int64_t *sel_idx, int64_t *m_out,
                  double *scores, double *mean_out);

// The batch in the wide range: the ragged finish on uniform descriptors (one
// group, k_collect_wide_ragged launches), whose output layout for equal n and
// f is this entry's
int finish_batch_wide(bk_ctx *c, Collect *k, const int64_t *orders, int64_t batch, int64_t n,
                      int64_t f, int64_t *sel_idx, double *scores, double *mean_out) {
    std::vector<int64_t> offsets((size_t)batch + 1), fs((size_t)batch, f);
    for (int64_t b = 0; b <= batch; ++b) offsets[(size_t)b] = b * n;
    return finish_ragged(c, k, orders, offsets.data(), fs.data(), batch, sel_idx, nullptr, scores,
                         mean_out);
}

}  // namespace

extern "C" {

int bk_collect_finish_batch(bk_ctx *c, const int64_t *orders, int64_t batch, int64_t n, int64_t f,
                            int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out) {
    // the shape checks first: they need no context, so they work with no GPU present
    if (batch < 1) return fail(BK_EINVAL, "need batch >= 1 (batch=%lld)", (long long)batch);
    if (batch > BK_MAX_BATCH)
        return fail(BK_ENOTSUP, "batch=%lld exceeds BK_MAX_BATCH=%d", (long long)batch, BK_MAX_BATCH);
    if (!c) return fail(BK_EINVAL, "null context");
    if (!orders) return fail(BK_EINVAL, "null orders");
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_finish_batch");
    if (!k) return BK_EINVAL;
    if (n < 1 || n > k->count)
        return fail(BK_EINVAL, "bk_collect_finish_batch: n=%lld, %lld rows collected",
                    (long long)n, (long long)k->count);
    CHK(bk_check_args(n, k->d, f));
    {
        std::vector<int64_t> seen((size_t)k->count, 0);
        for (int64_t b = 0; b < batch; ++b) CHK(check_order(orders + b * n, n, k->count, seen, b));
    }
    DeviceGuard dg(c->device);
    if (batch > 1 && small_ok(c, k->store.p, k->dtype, n, k->d, k->ld))
        CHK(finish_batch_small(c, k, orders, batch, n, f, sel_idx, scores, mean_out));
    else if (batch > 1 && wide_ok(c, n, k->d, mean_out != nullptr))
        CHK(finish_batch_wide(c, k, orders, batch, n, f, sel_idx, scores, mean_out));
    else
        CHK(finish_batch_loop(c, k, orders, batch, n, f, sel_idx, scores, mean_out));
    if (m_out) *m_out = n - f;
    return BK_OK;
}

}  // extern "C"

namespace {

constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// bk_collect_finish_ragged past its checks.  The problems within
// k_collect_small's range go by NB = ceil(n_b / 16) into buckets, and each
// bucket of two or more runs as k_collect_small_ragged<T, NB> launches of W <=
// SMALL_BATCH_MAX_W problems (bk_collect_ragged.hip): small_rank_sum<NB>,
// collect_row<NB> and small_mean<NB> take their summation shapes from NB and
// the single finish launches with the problem's own NB, so only the same
// instantiation gives the single finish's bits.  The descriptors, the launches'
// segment starts and the 16-bit slots go up in ONE copy from pinned staging;
// the kernel writes every output at its caller-order position in device arrays
// shaped like the caller's, which come back whole after the last launch.  Every
// other problem, and a bucket's only one, then runs the single finish straight
// into the caller's arrays, its record into the host side of the batch record
// store at the caller's index (finish_one_of_batch).  The buffers, the read-back
// and the closing bookkeeping are the batched finish's (batch_buffers,
// batch_readback, batch_close; both entries are synchronous and leave the lines
// zero).
int finish_ragged(bk_ctx *c, Collect *k, const int64_t *orders, const int64_t *offsets,
                  const int64_t *fs, int64_t batch, int64_t *sel_idx, int64_t *m_out,
                  double *scores, double *mean_out) {
    const int64_t d = k->d;
    const hipStream_t st = c->stream;
    const size_t ub = (size_t)batch;
    std::vector<int64_t> selo(ub + 1, 0);  // problem b's sel at sum_{c<b} m_c
    for (int64_t b = 0; b < batch; ++b)
        selo[(size_t)b + 1] = selo[(size_t)b] + (offsets[b + 1] - offsets[b]) - fs[b];
    // the wide range (bk_set_collect_wide): the same grouping, the launches
    // k_collect_wide_ragged's, bounded by the mean bytes a launch writes too
    const bool wide = wide_ok(c, 1, d, mean_out != nullptr);
    int64_t maxw = SMALL_BATCH_MAX_W;
    if (wide && mean_out) {
        const int64_t fit = (int64_t)(wide_out_bytes() / ((size_t)d * sizeof(double)));
        maxw = fit < 1 ? 1 : fit < maxw ? fit : maxw;
    }
    std::vector<int64_t> bucket[9], single;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (small_ok(c, k->store.p, k->dtype, n, d, k->ld) || wide_ok(c, n, d, mean_out != nullptr))
            bucket[(n + 15) / 16].push_back(b);
        else
            single.push_back(b);
    }
    struct Launch {
        int NB, W;
        size_t first, seg;  // its first descriptor; its segment starts (in int32s)
    };
    std::vector<Launch> launches;
    std::vector<int64_t> kern;  // the kernel's problems, in launch order
    size_t nseg = 0, nslots = 0;
    int maxW = 0;
    for (int NB = 1; NB <= 8; ++NB) {
        const std::vector<int64_t> &bk = bucket[NB];
        if (bk.size() == 1) single.push_back(bk[0]);
        if (bk.size() < 2) continue;
        for (size_t b0 = 0; b0 < bk.size(); b0 += (size_t)maxw) {
            const int w = (int)(bk.size() - b0 < (size_t)maxw ? bk.size() - b0 : (size_t)maxw);
            launches.push_back({NB, w, kern.size(), nseg});
            nseg += (size_t)w + 2;
            if (w > maxW) maxW = w;
            for (int q = 0; q < w; ++q) {
                kern.push_back(bk[b0 + q]);
                nslots += (size_t)(offsets[bk[b0 + q] + 1] - offsets[bk[b0 + q]]);
            }
        }
    }
    std::vector<double> recs(ub * MARGIN_WORDS);
    if (!launches.empty()) {
        const int C = !mean_out ? 1 : wide ? collect_wide_items(d) : (int)((d + 63) / 64);
        // the staging block: descriptors | segment starts | 16-bit slots
        const size_t off_seg = up16(kern.size() * sizeof(RaggedDesc));
        const size_t off_ord = up16(off_seg + nseg * sizeof(int32_t));
        const size_t sbytes = off_ord + nslots * sizeof(uint16_t);
        CHK(batch_buffers(c, k, "bk_collect_finish_ragged", batch, maxW, sbytes,
                          (size_t)offsets[batch], (size_t)selo[ub], mean_out != nullptr));
        Drain drain{st};
        char *hs = (char *)k->b_horder.p;
        RaggedDesc *hd = (RaggedDesc *)hs;
        int32_t *hseg = (int32_t *)(hs + off_seg);
        uint16_t *ho = (uint16_t *)(hs + off_ord);
        std::vector<int> lead(launches.size());
        {
            int64_t at = 0;  // the slots packed in launch order
            int32_t nn[SMALL_BATCH_MAX_W];
            for (size_t l = 0; l < launches.size(); ++l) {
                const Launch &L = launches[l];
                for (int q = 0; q < L.W; ++q) {
                    const int64_t b = kern[L.first + q], n = offsets[b + 1] - offsets[b];
                    RaggedDesc &r = hd[L.first + q];
                    r.n = nn[q] = (int32_t)n;
                    r.f = (int32_t)fs[b];
                    r.m = (int32_t)(n - fs[b]);
                    r.idx = (int32_t)b;
                    r.ord = at;
                    r.sc = offsets[b];
                    r.so = selo[(size_t)b];
                    for (int64_t i = 0; i < n; ++i)  // validated: < count <= 65,536
                        ho[at + i] = (uint16_t)orders[offsets[b] + i];
                    at += n;
                }
                ragged_seg_build(nn, L.W, C, hseg + L.seg);
                lead[l] = L.W > 1 ? hseg[L.seg + 2] - C : hseg[L.seg + 1];
            }
        }
        CHK(timed(c, BK_K_H2D, [&] {
            return hipMemcpyAsync(k->b_order.p, hs, sbytes, hipMemcpyHostToDevice, st);
        }));
        const char *ds = (const char *)k->b_order.p;
        double *dsc = (double *)k->b_scores.p, *ddg = (double *)k->b_diag.p;
        double *dmean = mean_out ? (double *)k->b_mean.p : nullptr;
        int64_t *dsel = (int64_t *)k->b_sel.p;
        for (size_t l = 0; l < launches.size(); ++l) {
            const Launch &L = launches[l];
            const uint64_t spin = next_spin(c);
            CHK(timed(c, BK_K_SMALL, [&] {
                return (wide ? launch_collect_wide_ragged : launch_collect_small_ragged)(
                    k->store.p, k->dtype, k->ld, L.W, L.NB, d, (const double *)k->G.p,
                    (const RaggedDesc *)ds + L.first, (const int32_t *)(ds + off_seg) + L.seg,
                    hseg[L.seg + L.W + 1], lead[l], (const uint16_t *)(ds + off_ord), dsc, ddg,
                    dsel, dmean, (double *)c->batch_rec.p, (unsigned *)k->b_ctr.p, c->num_cu, st,
                    spin);
            }));
        }
        // whole arrays, as the uniform entry's: the single finishes below fill
        // their own positions afterwards
        CHK(batch_readback(c, k, batch, (size_t)offsets[batch], (size_t)selo[ub], recs.data(),
                           sel_idx, scores, mean_out));
        drain.armed = false;
    }
    for (const int64_t b : single)
        CHK(finish_one_of_batch(c, k, orders + offsets[b], offsets[b + 1] - offsets[b], fs[b],
                                sel_idx + selo[(size_t)b], scores ? scores + offsets[b] : nullptr,
                                mean_out ? mean_out + b * d : nullptr,
                                recs.data() + (size_t)b * MARGIN_WORDS));
    if (m_out)
        for (int64_t b = 0; b < batch; ++b) m_out[b] = offsets[b + 1] - offsets[b] - fs[b];
    c->batch_rec_h.swap(recs);
    return batch_close(c, batch);
}

}  // namespace

extern "C" {

int bk_collect_finish_ragged(bk_ctx *c, const int64_t *orders, const int64_t *offsets,
                             const int64_t *fs, int64_t batch, int64_t *sel_idx, int64_t *m_out,
                             double *scores, double *mean_out) {
    // the shape checks first: they need no context, so they work with no GPU present
    if (batch < 1) return fail(BK_EINVAL, "need batch >= 1 (batch=%lld)", (long long)batch);
    if (batch > BK_MAX_BATCH)
        return fail(BK_ENOTSUP, "batch=%lld exceeds BK_MAX_BATCH=%d", (long long)batch, BK_MAX_BATCH);
    if (!c) return fail(BK_EINVAL, "null context");
    if (!orders) return fail(BK_EINVAL, "null orders");
    if (!offsets) return fail(BK_EINVAL, "null offsets");
    if (!fs) return fail(BK_EINVAL, "null fs");
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    Collect *k = begun(c, "bk_collect_finish_ragged");
    if (!k) return BK_EINVAL;
    if (offsets[0] != 0)
        return fail(BK_EINVAL, "bk_collect_finish_ragged: offsets[0] = %lld, not 0",
                    (long long)offsets[0]);
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t lo = offsets[b], hi = offsets[b + 1];  // lo >= 0: every offset before passed
        if (hi <= lo || (uint64_t)hi - (uint64_t)lo > (uint64_t)k->count)
            return fail(BK_EINVAL,
                        "problem %lld: n = offsets[%lld] - offsets[%lld] = %lld, %lld rows collected",
                        (long long)b, (long long)b + 1, (long long)b,
                        (long long)((uint64_t)hi - (uint64_t)lo), (long long)k->count);
    }
    for (int64_t b = 0; b < batch; ++b) {
        const int st = bk_check_args(offsets[b + 1] - offsets[b], k->d, fs[b]);
        if (st != BK_OK) {
            const std::string why = g_err;
            return fail(st, "problem %lld: %s", (long long)b, why.c_str());
        }
    }
    {
        std::vector<int64_t> seen((size_t)k->count, 0);
        for (int64_t b = 0; b < batch; ++b)
            CHK(check_order(orders + offsets[b], offsets[b + 1] - offsets[b], k->count, seen, b));
    }
    DeviceGuard dg(c->device);
    return finish_ragged(c, k, orders, offsets, fs, batch, sel_idx, m_out, scores, mean_out);
}

int bk_collect_wide_arrive_item(int64_t rows, int64_t d, int dtype, int64_t n, int mean,
                                int64_t item, int *kind, int *a, int *b, int64_t counts[4]) {
    if (!kind || !a || !b || !counts) return fail(BK_EINVAL, "null kind / a / b / counts");
    WideArriveQueue q;
    if (!wide_arrive_queue(q, rows, d, dtype, n, mean != 0))
        return fail(BK_EINVAL,
                    "need 1 <= rows <= 128, 1 <= n <= 128, a dtype and at most %d chunks of a row "
                    "(rows=%lld n=%lld d=%lld dtype=%d)",
                    WIDE_ARRIVE_MAX_B, (long long)rows, (long long)n, (long long)d, dtype);
    const int64_t total = (int64_t)q.nB + q.nR + q.nS + q.nM;
    if (item < 0 || item >= total)
        return fail(BK_EINVAL, "item %lld outside the queue (0..%lld)", (long long)item,
                    (long long)total - 1);
    counts[0] = q.nB;
    counts[1] = q.nR;
    counts[2] = q.nS;
    counts[3] = q.nM;
    wide_arrive_decode(q, (int)rows, (int)item, *kind, *a, *b);
    return BK_OK;
}

int bk_ragged_queue_item(const int32_t *n, int W, int C, int64_t item, int *p, int *it) {
    if (!n || !p || !it) return fail(BK_EINVAL, "null n / p / it");
    if (W < 1 || W > SMALL_BATCH_MAX_W || C < 1)
        return fail(BK_EINVAL, "need 1 <= W <= %d and C >= 1 (W=%d C=%d)", SMALL_BATCH_MAX_W, W, C);
    for (int j = 0; j < W; ++j)
        if (n[j] < 1 || n[j] > 128) return fail(BK_EINVAL, "n[%d] = %d outside 1..128", j, (int)n[j]);
    std::vector<int32_t> seg((size_t)W + 2);
    ragged_seg_build(n, W, C, seg.data());
    if (item < 0 || item >= seg[(size_t)W + 1])
        return fail(BK_EINVAL, "item %lld outside the queue (0..%d)", (long long)item,
                    (int)seg[(size_t)W + 1] - 1);
    ragged_queue_decode(seg.data(), W, C, (int)item, *p, *it);
    return BK_OK;
}

}  // extern "C"
