// bk_host.hip -- the host-staged entries (bk_multikrum, bk_multikrum_rows,
// bk_multikrum_noised): the batch crosses PCIe in column chunks under the Gram,
// the row-fed entry packs the caller's rows on a thread pool first, and the
// deployed shapes (n <= 128) take one copy and one launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "bk_ctx.h"
#include "bk_hostpool.h"

namespace {

// the host entries' copy stream and its five events, created once: into locals,
// published together (a half-built set would break every later host call)
int ensure_copy_stream(bk_ctx *c) {
    if (c->copy) return BK_OK;
    hipStream_t cs = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        if (cs) (void)hipStreamDestroy(cs);
        return fail(BK_EHIP, "copy stream / events: %s", hipGetErrorString(e));
    }
    c->copy = cs;
    c->ev_go = ev[0];
    c->ev_cp[0] = ev[1];
    c->ev_cp[1] = ev[2];
    c->ev_use[0] = ev[3];
    c->ev_use[1] = ev[4];
    return BK_OK;
}

// The host entries' column chunk width: ~BK_STAGE_CHUNK_BYTES (default 256
// MiB) of the batch plus its k noise vectors per chunk, a multiple of 64
// columns (16-B aligned chunk starts), at most 64 chunks (every chunk writes
// and adds one packed partial Gram -- n^2/2 doubles, 1 GiB at n = 16384 --
// which must stay small against its copy).  bk_multikrum and
// bk_multikrum_rows chunk alike, so their chunk Grams sum in the same order.
int64_t host_chunk_cols(int64_t n, size_t es, int64_t k, int64_t d) {
    int64_t cap = (int64_t)256 << 20;
    if (const char *v = getenv("BK_STAGE_CHUNK_BYTES")) cap = atoll(v) > 0 ? atoll(v) : cap;
    const int64_t col_bytes = n * (int64_t)es + n * k * (int64_t)sizeof(double);
    int64_t W = cap / col_bytes;
    W = W < (d + 63) / 64 ? (d + 63) / 64 : W;
    W = W < 64 ? 64 : (W + 63) / 64 * 64;
    return W >= d ? d : W;
}

}  // namespace

namespace bk {

// Host entries (bk_multikrum, bk_multikrum_noised): the batch crosses PCIe in
// column chunks on a copy stream, and each chunk's partial Gram (K1 + K1b,
// after K6 when noise is applied) runs on the compute stream while the next
// chunk is in flight.  The Gram is additive over columns, so only the last
// chunk's K1 and the finish remain after the copies; the chunk partials are
// added to a running sum in chunk order (deterministic).  Noise: vector j of update i at
// noise + (i*k + j) * noise_ld, staged per chunk in a 2-slot device ring.
// On return (async) the device batch dX (row stride dld) is complete and
// noised and U holds the full packed Gram; pl describes it for stage_finish.
int stage_host_pipelined(bk_ctx *c, const void *X, int64_t ld, int dtype, const double *noise,
                         int64_t k, int64_t noise_ld, int64_t n, int64_t d, char *dX,
                         int64_t dld, double *U, Plan &pl) {
    const size_t es = esize(dtype);
    CHK(ensure_copy_stream(c));
    const int64_t W = host_chunk_cols(n, es, k, d);
    const int64_t C = (d + W - 1) / W;
    const size_t usz = (size_t)bk_upper_elems(n);
    double *P = nullptr;
    if (C > 1) {
        CHK(ensure(c->Ug, usz * sizeof(double)));
        P = (double *)c->Ug.p;
    }
    double *ring = nullptr;
    if (k > 0) {
        CHK(ensure(c->noise, (size_t)2 * n * k * W * sizeof(double)));
        ring = (double *)c->noise.p;
    }
    // on an error return, copies already queued may still read the caller's
    // host buffers: drain both streams before handing control back
    HostDrain drain{c};
    // earlier work on the compute stream may still read the batch / the ring
    HIPCHK(hipEventRecord(c->ev_go, c->stream));
    HIPCHK(hipStreamWaitEvent(c->copy, c->ev_go, 0));
    for (int64_t ch = 0; ch < C; ++ch) {
        const int64_t c0 = ch * W, wc = d - c0 < W ? d - c0 : W;
        const int s = (int)(ch & 1);
        double *slot = ring ? ring + (size_t)s * n * k * W : nullptr;
        if (ch >= 2 && k > 0) HIPCHK(hipStreamWaitEvent(c->copy, c->ev_use[s], 0));
        HIPCHK(hipMemcpy2DAsync(dX + c0 * es, (size_t)dld * es, (const char *)X + c0 * es,
                                (size_t)ld * es, (size_t)wc * es, (size_t)n,
                                hipMemcpyHostToDevice, c->copy));
        if (k > 0)
            HIPCHK(hipMemcpy2DAsync(slot, (size_t)wc * 8, noise + c0, (size_t)noise_ld * 8,
                                    (size_t)wc * 8, (size_t)(n * k), hipMemcpyHostToDevice,
                                    c->copy));
        HIPCHK(hipEventRecord(c->ev_cp[s], c->copy));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_cp[s], 0));
        double *xc = (double *)(dX + c0 * es);
        if (k > 0) {
            CHK(timed(c, BK_K_NOISE, [&] {
                return launch_noise(xc, dld, n, wc, slot, k, wc, xc, dld, c->num_cu, c->stream);
            }));
            HIPCHK(hipEventRecord(c->ev_use[s], c->stream));
        }
        // chunk 0 straight into U, later chunks added in chunk order
        CHK(stage_gram(c, dX + c0 * es, dtype, n, wc, dld, ch == 0 ? U : P, pl));
        if (ch > 0) HIPCHK(launch_add_upper(U, P, (int64_t)usz, c->stream));
    }
    pl.d = d;
    drain.armed = false;
    return BK_OK;
}

}  // namespace bk

namespace {

// K2..K4 on a batch staged by stage_host_pipelined, then the outputs back to
// the caller's host arrays (bk_multikrum, bk_multikrum_noised)
int run_host_outputs(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t dld,
                     int64_t f, const double *U, const Plan &pl, int64_t *sel_idx,
                     int64_t *m_out, double *scores, double *mean_out) {
    HostDrain drain{c};
    const int64_t m = n - f;
    CHK(ensure(c->sel, (size_t)n * sizeof(int64_t)));
    CHK(ensure(c->scores, (size_t)n * sizeof(double)));
    if (mean_out) CHK(ensure(c->mean, (size_t)d * sizeof(double)));
    int64_t *dsel = (int64_t *)c->sel.p;
    double *dsc = (double *)c->scores.p;
    double *dmean = mean_out ? (double *)c->mean.p : nullptr;
    CHK(stage_finish(c, U, pl, dX, dtype, n, d, dld, f, dsel, dsc, dmean));
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(sel_idx, dsel, (size_t)m * sizeof(int64_t),
                                      hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && scores)
            e = hipMemcpyAsync(scores, dsc, (size_t)n * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream);
        if (e == hipSuccess && mean_out)
            e = hipMemcpyAsync(mean_out, dmean, (size_t)d * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream);
        return e;
    }));
    HIPCHK(wait_stream(c));
    drain.armed = false;
    CHK(check_margin_readback(c));
    if (m_out) *m_out = m;
    return BK_OK;
}

// Host batches of Biscotti's deployed shapes (n <= 128: configs A and B, the
// mnist and creditcard verifiers) take the one-launch k_small / k_tiny path:
// ONE H2D of the 16-B-padded batch on the compute stream (<= 32 MiB: no column
// chunks, no copy stream), the noise added in place by K6 when the verifier
// noises the batch itself, the kernel, then the outputs and the margin record
// back, one synchronize.  The device-resident entry's arithmetic, so the same
// bits.  where == BK_DEVICE skips the copy, and so does a pinned batch that
// k_tiny reads over PCIe itself (below).
int run_host_small(bk_ctx *c, const void *X, int where, int64_t ld, int dtype, const double *noise,
                   int64_t k, int64_t noise_ld, int64_t n, int64_t d, int64_t f, int64_t *sel_idx,
                   int64_t *m_out, double *scores, double *mean_out, double *noised_out,
                   int64_t out_ld) {
    const size_t es = esize(dtype);
    const int64_t m = n - f;
    HostDrain drain{c};
    const void *dX = X;
    int64_t dld = ld;
    // a batch k_tiny takes whole (n <= 16, d <= 128: config A, a few KB) is
    // read by the kernel itself straight from the caller's pinned memory over
    // PCIe: no H2D copy, whose DMA set-up (~20 us) was most of the call
    // (BK_TINY_ZERO_COPY=0 copies it as before, for A/B)
    static const bool tiny_zc = [] {
        const char *e = getenv("BK_TINY_ZERO_COPY");
        return !(e && atoi(e) == 0);
    }();
    bool zero_copy = false;
    if (where == BK_HOST_PINNED && k == 0 && !noised_out && tiny_zc && tiny_ok((int)n, d) &&
        !probe_env("BK_SMALL_TRACE")) {
        void *hp = nullptr;
        if (hipHostGetDevicePointer(&hp, const_cast<void *>(X), 0) == hipSuccess && hp) {
            dX = hp;
            zero_copy = true;
        } else {
            (void)hipGetLastError();  // not mapped (pinned by other means): copy it
        }
    }
    // BK_SMALL_PIPE=<chunks> (A/B; default 0): the copy in that many column
    // chunks on the copy stream, each chunk's G items launched on the compute
    // stream as soon as it has landed (an event, no spinning), then one S + M
    // launch -- the same items and partials as the one-launch call, the same
    // bits.  Measured at config B (r4, tools/host_entry_ab.py): 0.157 ms per
    // call with one copy, 0.201 with 2 chunks, 0.234 with 4 -- a strided
    // column-chunk H2D and its launch cost more than the Gram they hide
    // (~14 us), so the one copy + one launch stays the default
    static const int pipe_env = [] {
        const char *e = getenv("BK_SMALL_PIPE");
        return e ? atoi(e) : 0;
    }();
    const SmallPlan sp = small_plan((int)n, d, c->num_cu);
    int nc = 0;
    if (where != BK_DEVICE && !zero_copy && k == 0 && !noised_out && !tiny_ok((int)n, d) &&
        !probe_env("BK_SMALL_TRACE") && pipe_env >= 2 && sp.P >= 2 * pipe_env)
        nc = pipe_env;
    if (nc) {
        const int64_t epg = (int64_t)(16 / es);
        dld = (d + epg - 1) / epg * epg;
        CHK(ensure(c->X, (size_t)n * dld * es));
        CHK(ensure_copy_stream(c));
        char *dx = (char *)c->X.p;
        // earlier work on the compute stream may still read the device batch
        HIPCHK(hipEventRecord(c->ev_go, c->stream));
        HIPCHK(hipStreamWaitEvent(c->copy, c->ev_go, 0));
        for (int q = 0; q < nc; ++q) {
            const int a0 = (int)((int64_t)sp.P * q / nc), a1 = (int)((int64_t)sp.P * (q + 1) / nc);
            const int64_t c0 = (int64_t)a0 * sp.kc, c1 = std::min<int64_t>((int64_t)a1 * sp.kc, d);
            HIPCHK(hipMemcpy2DAsync(dx + c0 * es, (size_t)dld * es, (const char *)X + c0 * es,
                                    (size_t)ld * es, (size_t)(c1 - c0) * es, (size_t)n,
                                    hipMemcpyHostToDevice, c->copy));
            HIPCHK(hipEventRecord(c->ev_cp[q & 1], c->copy));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_cp[q & 1], 0));
            CHK(run_small(c, dx, dtype, n, d, dld, f, nullptr, nullptr, nullptr, nullptr, nullptr,
                          a0, a1 - a0, false));
        }
        dX = dx;
    }
    if (where != BK_DEVICE && !zero_copy && !nc) {
        const int64_t epg = (int64_t)(16 / es);
        dld = (d + epg - 1) / epg * epg;
        CHK(ensure(c->X, (size_t)n * dld * es));
        if (k > 0) CHK(ensure(c->noise, (size_t)n * k * d * sizeof(double)));
        CHK(timed(c, BK_K_H2D, [&] {
            // a contiguous batch (ld == d) whose rows are already 16-B
            // multiples (ld == dld): one linear copy.  A strided caller with
            // ld == dld != d (a numpy view X[:, :3] of an n x 4 array) takes
            // the 2-D copy: a linear n * d copy would shift every row after
            // the first
            hipError_t e = ld == dld && ld == d ? hipMemcpyAsync(c->X.p, X, (size_t)n * d * es,
                                                      hipMemcpyHostToDevice, c->stream)
                                     : hipMemcpy2DAsync(c->X.p, (size_t)dld * es, X,
                                                        (size_t)ld * es, (size_t)d * es, (size_t)n,
                                                        hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess && k > 0)
                e = hipMemcpy2DAsync(c->noise.p, (size_t)d * 8, noise, (size_t)noise_ld * 8,
                                     (size_t)d * 8, (size_t)(n * k), hipMemcpyHostToDevice,
                                     c->stream);
            return e;
        }));
        if (k > 0) {
            double *xd = (double *)c->X.p;
            CHK(timed(c, BK_K_NOISE, [&] {
                return launch_noise(xd, dld, n, d, (const double *)c->noise.p, k, d, xd, dld,
                                    c->num_cu, c->stream);
            }));
        }
        if (noised_out)
            HIPCHK(hipMemcpy2DAsync(noised_out, (size_t)out_ld * 8, c->X.p, (size_t)dld * 8,
                                    (size_t)d * 8, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        dX = c->X.p;
    }
    // the outputs {margin (16 doubles), sel (n), scores (n), mean (d)} are
    // written by the kernel itself into one mapped pinned block:
    // no device-to-host copy after the kernel (a D2H costs ~15 us of PCIe
    // round trip at config B, more than the 63 KB it moves), one synchronize,
    // then copied to the caller's arrays on the host
    constexpr size_t MPAD = HOUT_MPAD;
    CHK(ensure_hout(c, MPAD + 2 * (size_t)n + (mean_out ? (size_t)d : 0)));
    double *blk = c->hout_dev;
    int64_t *dsel = (int64_t *)(blk + MPAD);
    double *dmean = mean_out ? blk + MPAD + 2 * n : nullptr;
    CHK(run_small(c, dX, dtype, n, d, dld, f, dsel, nullptr, dmean, blk,
                  scores ? blk + MPAD + n : nullptr, 0, nc ? 0 : -1, true));
    HIPCHK(wait_stream(c));
    drain.armed = false;
    const double *h = (const double *)c->hout;
    c->margin_unchecked = 0;
    CHK(margin_status(h));
    memcpy(sel_idx, h + MPAD, (size_t)m * sizeof(int64_t));
    if (scores) memcpy(scores, h + MPAD + n, (size_t)n * sizeof(double));
    if (mean_out) memcpy(mean_out, h + MPAD + 2 * n, (size_t)d * sizeof(double));
    if (m_out) *m_out = m;
    return BK_OK;
}

// ---- the row-fed host entry (bk_multikrum_rows) ----------------------------
// Biscotti's verifier holds the batch as n separately allocated host rows
// (getTopKRUMIndex(deltas [][]float64), krum.go:100-166; each row a peer's
// RPC-decoded slice).  Before anything crosses PCIe the rows must be in
// pinned memory.  The cgo shim used to pack them serially into a pinned batch
// (one core, 4.3 GB at config D) and only then call bk_multikrum; here the
// packing runs on several host threads into a ring of pinned slots, and each
// slot's H2D (and the Gram of its columns) starts as soon as it is full.

// packing threads, the caller's included: bk_set_host_threads, else
// BK_HOST_THREADS, else min(8, the host's hardware threads) -- config D's
// pack keeps ahead of PCIe from 4 threads on (78-79 ms per call at 4, 8 and
// 16), and more threads only compete for the process's CPU share
int host_threads(const bk_ctx *c) {
    if (c->hthreads > 0) return c->hthreads;
    static const int def = [] {
        if (const char *v = getenv("BK_HOST_THREADS"))
            if (atoi(v) > 0) return std::min(atoi(v), 256);
        const unsigned hw = std::thread::hardware_concurrency();
        return (int)std::max(1u, std::min(8u, hw ? hw : 1u));
    }();
    return def;
}

// the context's worker pool (threads - 1 workers), or nullptr when the caller
// packs alone (one thread, or the workers could not be started)
bk::HostPool *get_pool(bk_ctx *c) {
    const int t = host_threads(c);
    if (c->hpool && c->hpool->workers() == t - 1) return c->hpool;
    delete c->hpool;
    c->hpool = nullptr;
    if (t <= 1) return nullptr;
    try {
        c->hpool = new bk::HostPool(t - 1);
    } catch (...) {
        c->hpool = nullptr;
    }
    return c->hpool;
}

// one packing job on the pool for the lifetime of this object: the pool's
// end() runs on every return path, so no worker still uses the job function
// (on the caller's stack) or writes into the stage after the entry returns
struct PoolJob {
    bk::HostPool *pool;
    PoolJob(bk::HostPool *p, int nitems, const std::function<void(int)> *fn) : pool(p) {
        if (pool) pool->begin(nitems, fn);
    }
    ~PoolJob() {
        if (pool) pool->end();
    }
};

// the pack's stores: non-temporal for the column-chunk ring (GBs streamed
// through it: the stores bypass the caches), cached memcpy for the small
// path's stage (<= 32 MiB, re-used every call: it stays in the L3, and r6's
// sweep at config B gave ~0.195 ms per call against ~0.205 non-temporal);
// BK_ROWS_COPY=nt|memcpy forces one (an A/B of the same bytes)
bool rows_copy_nt(bool dflt) {
    const char *e = getenv("BK_ROWS_COPY");
    if (e && strcmp(e, "memcpy") == 0) return false;
    if (e && strcmp(e, "nt") == 0) return true;
    return dflt;
}

// the pinned ring (grow-only; every call is synchronous, so no copy from the
// old ring is in flight when it is replaced)
int ensure_rows_stage(bk_ctx *c, size_t bytes) {
    if (c->rstage_bytes >= bytes) return BK_OK;
    if (c->rstage) (void)hipHostFree(c->rstage);
    c->rstage = nullptr;
    c->rstage_bytes = 0;
    HIPCHK(hipHostMalloc(&c->rstage, bytes, hipHostMallocPortable | hipHostMallocMapped));
    c->rstage_bytes = bytes;
    return BK_OK;
}

int ensure_rows_events(bk_ctx *c) {
    for (hipEvent_t &e : c->ev_rows)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return BK_OK;
}

// Column chunks of the batch through a ring of S <= 3 pinned slots: chunk ch
// (columns [ch W, ch W + W)) is packed by the pool into slot ch mod S (row
// blocks of ~2 MiB are the items), crosses PCIe on the copy stream into the
// device batch dX (row stride dld), and its partial Gram runs on the compute
// stream, as in stage_host_pipelined.  A slot is handed back to the packers
// when its copy has landed, so the packing of chunks ch + 1 .. ch + S - 1
// overlaps the copy of chunk ch.  The chunks are bk_multikrum's
// (host_chunk_cols), summed in the same order: every output is bitwise that of
// bk_multikrum on the rows packed into one pinned batch.
int stage_rows_pipelined(bk_ctx *c, const char *const *rows, int dtype, int64_t n, int64_t d,
                         char *dX, int64_t dld, double *U, Plan &pl) {
    const size_t es = esize(dtype);
    CHK(ensure_copy_stream(c));
    CHK(ensure_rows_events(c));
    const int64_t W = host_chunk_cols(n, es, 0, d);
    const int64_t C = (d + W - 1) / W;
    const int S = (int)std::min<int64_t>(C, 3);
    const size_t slot = (size_t)n * W * es;
    CHK(ensure_rows_stage(c, slot * S));
    const size_t usz = (size_t)bk_upper_elems(n);
    double *P = nullptr;
    if (C > 1) {
        CHK(ensure(c->Ug, usz * sizeof(double)));
        P = (double *)c->Ug.p;
    }
    // items: blocks of rb rows of one chunk, ~2 MiB each
    const int64_t rb = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)2 << 20) / (W * (int64_t)es)));
    const int64_t ipc = (n + rb - 1) / rb;
    std::unique_ptr<std::atomic<int64_t>[]> done(new std::atomic<int64_t>[C]);
    for (int64_t ch = 0; ch < C; ++ch) done[ch].store(0, std::memory_order_relaxed);
    char *stage = (char *)c->rstage;
    const bool nt = rows_copy_nt(true);
    const std::function<void(int)> fn = [&](int it) {
        const int64_t ch = it / ipc, r0 = (it % ipc) * rb, r1 = std::min(n, r0 + rb);
        const int64_t c0 = ch * W, wc = std::min(W, d - c0);
        char *sl = stage + (size_t)(ch % S) * slot;
        for (int64_t r = r0; r < r1; ++r)
            bk::copy_to_stage(sl + (size_t)r * wc * es, rows[r] + (size_t)c0 * es, (size_t)wc * es,
                              nt);
        _mm_sfence();
        done[ch].fetch_add(1, std::memory_order_release);
    };
    // on an error return, copies already queued may still read the stage and
    // write dX: drain both streams (after the pool has stopped, below)
    HostDrain drain{c};
    // earlier work on the compute stream may still read the device batch
    HIPCHK(hipEventRecord(c->ev_go, c->stream));
    HIPCHK(hipStreamWaitEvent(c->copy, c->ev_go, 0));
    bk::HostPool *pool = get_pool(c);
    PoolJob job(pool, (int)(C * ipc), &fn);
    if (pool) pool->release((int)(S * ipc));
    for (int64_t ch = 0; ch < C; ++ch) {
        const int64_t c0 = ch * W, wc = std::min(W, d - c0);
        const int s = (int)(ch % S);
        if (pool) {
            while (done[ch].load(std::memory_order_acquire) < ipc)
                if (!pool->help()) _mm_pause();
        } else {
            for (int64_t i = ch * ipc; i < (ch + 1) * ipc; ++i) fn((int)i);
        }
        HIPCHK(hipMemcpy2DAsync(dX + c0 * es, (size_t)dld * es, stage + (size_t)s * slot,
                                (size_t)wc * es, (size_t)wc * es, (size_t)n, hipMemcpyHostToDevice,
                                c->copy));
        HIPCHK(hipEventRecord(c->ev_rows[s], c->copy));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_rows[s], 0));
        CHK(stage_gram(c, dX + c0 * es, dtype, n, wc, dld, ch == 0 ? U : P, pl));
        if (ch > 0) HIPCHK(launch_add_upper(U, P, (int64_t)usz, c->stream));
        // chunk ch - 1's slot is free once its copy (queued before chunk ch's,
        // which keeps the copy engine busy meanwhile) has landed: chunk
        // ch - 1 + S goes into it
        if (ch >= 1 && ch - 1 + S < C) {
            HIPCHK(hipEventSynchronize(c->ev_rows[(ch - 1) % S]));
            if (pool) pool->release((int)((ch + S) * ipc));
        }
    }
    pl.d = d;
    drain.armed = false;
    return BK_OK;
}

// Biscotti's deployed shapes (n <= 128, d <= 32768: configs A and B) on the
// row-fed entry.  k_tiny's batches (n <= 16, d <= 128) are packed by the
// caller into the mapped pinned stage, which the kernel reads over PCIe (as
// bk_multikrum's pinned batches).  Larger ones are packed by the pool in
// row order into a stage laid out like the device batch (16-B rows), and
// each group of rows crosses PCIe as one linear copy on the compute stream
// as soon as it is packed (BK_ROWS_GROUPS groups, default 3, growing x1.5),
// so the copy engine starts after the first sixth of the pack instead of
// after all of it; then the one-launch k_small, as bk_multikrum's host path.
// (r6 sweep at config B, tools/rows_probe.py --sweep: every extra copy costs
// more than the pack it hides beyond 3-4 groups.)
int run_rows_small(bk_ctx *c, const char *const *rows, int dtype, int64_t n, int64_t d, int64_t f,
                   int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out) {
    const size_t es = esize(dtype);
    const int64_t epg = (int64_t)(16 / es);
    const int64_t dld = (d + epg - 1) / epg * epg;
    const size_t rowb = (size_t)dld * es;
    CHK(ensure_rows_stage(c, (size_t)n * rowb));
    char *stage = (char *)c->rstage;
    if (tiny_ok((int)n, d)) {
        for (int64_t r = 0; r < n; ++r) memcpy(stage + (size_t)r * rowb, rows[r], (size_t)d * es);
        return run_host_small(c, stage, BK_HOST_PINNED, dld, dtype, nullptr, 0, 0, n, d, f, sel_idx,
                              m_out, scores, mean_out, nullptr, 0);
    }
    const char *ge = getenv("BK_ROWS_GROUPS");
    const int groups_env = ge && atoi(ge) > 0 ? atoi(ge) : 3;
    CHK(ensure(c->X, (size_t)n * rowb));
    // items: ~128 KiB of rows each.  Groups grow geometrically (x1.5): the
    // copy engine starts after the first small group is packed, and each
    // later group is packed (by several threads, faster than PCIe drains
    // the stage) while the groups before it are in flight
    const int64_t ri = std::max<int64_t>(1, ((int64_t)128 << 10) / (d * (int64_t)es));
    const int64_t I = (n + ri - 1) / ri;
    const int64_t G = std::min<int64_t>(groups_env, I);
    std::vector<int64_t> gstart((size_t)G + 1);
    {
        double tot = 0, w = 1;
        for (int64_t g = 0; g < G; ++g, w *= 1.5) tot += w;
        double acc = 0;
        w = 1;
        gstart[0] = 0;
        for (int64_t g = 1; g <= G; ++g, w *= 1.5) {
            acc += w;
            gstart[(size_t)g] = std::max(gstart[(size_t)g - 1] + 1,
                                         std::min<int64_t>(I - (G - g), (int64_t)(I * acc / tot + 0.5)));
        }
        gstart[(size_t)G] = I;
    }
    std::unique_ptr<std::atomic<int64_t>[]> done(new std::atomic<int64_t>[G]);
    for (int64_t g = 0; g < G; ++g) done[g].store(0, std::memory_order_relaxed);
    const bool nt = rows_copy_nt(false);
    const std::function<void(int)> fn = [&](int it) {
        const int64_t r0 = it * ri, r1 = std::min(n, r0 + ri);
        for (int64_t r = r0; r < r1; ++r)
            bk::copy_to_stage(stage + (size_t)r * rowb, rows[r], (size_t)d * es, nt);
        _mm_sfence();
        int64_t g = 0;
        while (gstart[(size_t)g + 1] <= it) ++g;
        done[g].fetch_add(1, std::memory_order_release);
    };
    HostDrain drain{c};
    // debug (probe build): host timeline of the call, us from entry
    const bool trace = probe_env("BK_ROWS_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> tl;
    auto mark = [&] {
        if (trace)
            tl.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    {
        // a stage of <= 8 MiB (config B: 6.3 MB) is packed by the caller
        // alone: waking the pool costs more than it saves there (B, per call:
        // 0.195 ms with 1-4 packing threads, 0.217 with 8; bench e2e_rows)
        bk::HostPool *pool = (size_t)n * rowb > ((size_t)8 << 20) ? get_pool(c) : nullptr;
        PoolJob job(pool, (int)I, &fn);
        if (pool) pool->release((int)I);
        mark();
        char *dx = (char *)c->X.p;
        for (int64_t g = 0; g < G; ++g) {
            const int64_t need = gstart[(size_t)g + 1] - gstart[(size_t)g];
            if (pool) {
                while (done[g].load(std::memory_order_acquire) < need)
                    if (!pool->help()) _mm_pause();
            } else {
                for (int64_t i = gstart[(size_t)g]; i < gstart[(size_t)g + 1]; ++i) fn((int)i);
            }
            mark();
            const int64_t r0 = gstart[(size_t)g] * ri, r1 = std::min(n, gstart[(size_t)g + 1] * ri);
            CHK(timed(c, BK_K_H2D, [&] {
                return hipMemcpyAsync(dx + (size_t)r0 * rowb, stage + (size_t)r0 * rowb,
                                      (size_t)(r1 - r0) * rowb, hipMemcpyHostToDevice, c->stream);
            }));
            mark();
        }
    }
    mark();
    const int st = run_host_small(c, c->X.p, BK_DEVICE, dld, dtype, nullptr, 0, 0, n, d, f, sel_idx,
                                  m_out, scores, mean_out, nullptr, 0);
    mark();
    if (trace) {
        fprintf(stderr, "rows_trace G=%lld I=%lld:", (long long)G, (long long)I);
        for (double t : tl) fprintf(stderr, " %.1f", t);
        fprintf(stderr, "\n");
    }
    drain.armed = st != BK_OK;
    return st;
}

// the host entries' certified modes: a near tie of an approximate Gram re-runs
// exact from the device-resident batch dX (row stride dld), whose outputs
// replace the first run's in the caller's arrays
int host_certified_rerun(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t dld,
                         int64_t f, double *U, int64_t *sel_idx, int64_t *m_out, double *scores,
                         double *mean_out) {
    if (!certified(c, dtype)) return BK_OK;
    double mg[MARGIN_WORDS];
    CHK(read_margin(c, mg));
    if (!(mg[2] != 0.0 && mg[8] > 0x1p-53)) return BK_OK;
    c->force_exact = 1;
    Plan pl2;
    int st = stage_gram(c, dX, dtype, n, d, dld, U, pl2);
    if (st == BK_OK)
        st = run_host_outputs(c, dX, dtype, n, d, dld, f, U, pl2, sel_idx, m_out, scores, mean_out);
    c->force_exact = 0;
    if (st == BK_OK) ++c->certified_reruns;
    return st;
}

}  // namespace

extern "C" {

int bk_multikrum(bk_ctx *c, const void *X, int where, int dtype, int64_t n, int64_t d, int64_t ld,
                 int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out) {
    CHK(check_common(c, X, dtype, n, d, ld));
    CHK(bk_check_args(n, d, f));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    // n <= 128: one copy and the one-launch path (always exact: no certified re-run)
    if (small_ok(c, X, dtype, n, d, ld))
        return run_host_small(c, X, where, ld, dtype, nullptr, 0, 0, n, d, f, sel_idx, m_out,
                              scores, mean_out, nullptr, 0);
    const size_t es = esize(dtype);
    const void *dX = X;
    int64_t dld = ld;
    CHK(ensure(c->U, (size_t)bk_upper_elems(n) * sizeof(double)));
    double *U = (double *)c->U.p;
    Plan pl;
    if (where != BK_DEVICE) {
        // device rows padded to 16 B so K1 v3 (global_load_lds granules) always applies
        const int64_t epg = (int64_t)(16 / es);
        dld = (d + epg - 1) / epg * epg;
        CHK(ensure(c->X, (size_t)n * dld * es));
        CHK(stage_host_pipelined(c, X, ld, dtype, nullptr, 0, 0, n, d, (char *)c->X.p, dld, U,
                                 pl));
        dX = c->X.p;
    } else {
        CHK(stage_gram(c, dX, dtype, n, d, dld, U, pl));
    }
    CHK(run_host_outputs(c, dX, dtype, n, d, dld, f, U, pl, sel_idx, m_out, scores, mean_out));
    return host_certified_rerun(c, dX, dtype, n, d, dld, f, U, sel_idx, m_out, scores, mean_out);
}

int bk_multikrum_rows(bk_ctx *c, const void *const *rows, int dtype, int64_t n, int64_t d,
                      int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores,
                      double *mean_out) {
    CHK(check_common(c, rows, dtype, n, d, d));
    CHK(bk_check_args(n, d, f));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    for (int64_t i = 0; i < n; ++i)
        if (!rows[i]) return fail(BK_EINVAL, "null row %lld", (long long)i);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    const char *const *R = (const char *const *)rows;
    if (small_ok(c, nullptr, dtype, n, d, d))
        return run_rows_small(c, R, dtype, n, d, f, sel_idx, m_out, scores, mean_out);
    const size_t es = esize(dtype);
    const int64_t epg = (int64_t)(16 / es);
    const int64_t dld = (d + epg - 1) / epg * epg;
    CHK(ensure(c->X, (size_t)n * dld * es));
    CHK(ensure(c->U, (size_t)bk_upper_elems(n) * sizeof(double)));
    double *U = (double *)c->U.p;
    Plan pl;
    CHK(stage_rows_pipelined(c, R, dtype, n, d, (char *)c->X.p, dld, U, pl));
    CHK(run_host_outputs(c, c->X.p, dtype, n, d, dld, f, U, pl, sel_idx, m_out, scores, mean_out));
    return host_certified_rerun(c, c->X.p, dtype, n, d, dld, f, U, sel_idx, m_out, scores, mean_out);
}

int bk_set_host_threads(bk_ctx *c, int threads) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (threads < 0 || threads > 256) return fail(BK_EINVAL, "threads=%d out of [0, 256]", threads);
    std::lock_guard<std::mutex> lk(c->mu);
    c->hthreads = threads;
    return BK_OK;
}

// the noise application fused into the H2D staging of
// the verifier batch.  Rows go over in chunks on a copy stream (Delta rows
// straight into the padded device batch, their k noise vectors into a 2-slot
// ring); K6 adds each chunk's noise in place on the compute stream while the
// next chunk is in flight.  No host pass over n*d, and no n*k*d device buffer.
int bk_multikrum_noised(bk_ctx *c, const double *delta, int64_t ld, const double *noise,
                        int64_t k, int64_t noise_ld, int where, int64_t n, int64_t d, int64_t f,
                        int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out,
                        double *noised_out, int64_t out_ld) {
    CHK(check_common(c, delta, BK_F64, n, d, ld));
    CHK(bk_check_args(n, d, f));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    if (where != BK_HOST && where != BK_HOST_PINNED)
        return fail(BK_EINVAL, "bad where=%d (host batches only; device-resident batches use "
                               "bk_noise_apply_device + bk_multikrum_device)", where);
    if (k < 0) return fail(BK_EINVAL, "k=%lld < 0", (long long)k);
    if (k > 0 && !noise) return fail(BK_EINVAL, "null noise with k=%lld", (long long)k);
    if (k > 0 && noise_ld < d) return fail(BK_EINVAL, "noise_ld=%lld < d", (long long)noise_ld);
    if (noised_out && out_ld < d) return fail(BK_EINVAL, "out_ld=%lld < d", (long long)out_ld);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    // n <= 128: one copy of the batch and its noise, K6, the one-launch path
    if (small_ok(c, delta, BK_F64, n, d, ld))
        return run_host_small(c, delta, where, ld, BK_F64, k > 0 ? noise : nullptr, k, noise_ld, n,
                              d, f, sel_idx, m_out, scores, mean_out, noised_out, out_ld);
    const int64_t dld = (d + 1) / 2 * 2;  // 16-B rows: K1 v3 applies
    CHK(ensure(c->X, (size_t)n * dld * sizeof(double)));
    double *dX = (double *)c->X.p;
    CHK(ensure(c->U, (size_t)bk_upper_elems(n) * sizeof(double)));
    double *U = (double *)c->U.p;
    Plan pl;
    // armed until the outputs have landed: on any error return, copies still
    // queued may read delta / noise or write noised_out
    HostDrain drain{c};
    // k = 0: no noisers, NoisedDelta = Delta (main.go:1599-1602)
    CHK(stage_host_pipelined(c, delta, ld, BK_F64, k > 0 ? noise : nullptr, k, noise_ld, n, d,
                             (char *)dX, dld, U, pl));
    if (noised_out)
        HIPCHK(hipMemcpy2DAsync(noised_out, (size_t)out_ld * 8, dX, (size_t)dld * 8,
                                (size_t)d * 8, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    CHK(run_host_outputs(c, dX, BK_F64, n, d, dld, f, U, pl, sel_idx, m_out, scores, mean_out));
    drain.armed = false;
    return BK_OK;
}

}  // extern "C"
