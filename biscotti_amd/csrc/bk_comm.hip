// bk_comm.hip -- the RCCL sharded path (bk_comm_*, bk_multikrum_sharded_device):
// every rank's partial Gram of its column shard, the ranks' status agreement,
// the exchange -- whole, or in pieces overlapped with the Gram -- and the finish.
#include <emmintrin.h>
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "bk_ctx.h"

namespace {

ScoreSplit score_split(const bk_ctx *c, int64_t n) {
    ScoreSplit s;
    if (!c->comm || c->split_min_n <= 0 || n < c->split_min_n || !scores_transposed((int)n))
        return s;
    if (c->nranks > 1) {
        s.mode = SPLIT_RCCL;
        s.parts = c->nranks;
        s.part = c->rank;
    } else if (c->test_split_scores > 1) {
        s.mode = SPLIT_TEST;
        s.parts = c->test_split_scores;
    } else if (c->emu_split_scores > 1) {
        s.mode = SPLIT_EMU;
        s.parts = c->emu_split_scores;
    }
    return s;
}

}  // namespace

extern "C" {

int bk_comm_unique_id(void *id_out) {
    if (!id_out) return fail(BK_EINVAL, "null id");
    static_assert(sizeof(ncclUniqueId) == BK_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    RCCLCHK(ncclGetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return BK_OK;
}

int bk_comm_init(bk_ctx *c, int nranks, int rank, const void *id) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(BK_EINVAL, "bad comm_init arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (c->comm) {
        (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
    }
    // the sharded entry's status agreement word, before the communicator (an
    // allocation failure then fails this rank's init, not a later collective)
    CHK(ensure(c->status, 4 * sizeof(double)));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    RCCLCHK(ncclCommInitRank(&c->comm, nranks, uid, rank));
    c->nranks = nranks;
    c->rank = rank;
    c->agreed_n = c->agreed_f = -1;  // the next sharded call agrees again
    return BK_OK;
}

int bk_comm_set_mode(bk_ctx *c, int mode) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (mode < 0 || mode > 2) return fail(BK_EINVAL, "bad exchange mode %d", mode);
    std::lock_guard<std::mutex> lk(c->mu);
    c->deterministic = mode == 1 ? 1 : 0;
    int k = 2;
    if (const char *v = getenv("BK_OVERLAP_PIECES")) k = atoi(v);
    c->overlap = mode == 2 ? std::max(2, std::min(8, k)) : 0;
    return BK_OK;
}

namespace {
// the communication stream of the overlapped exchange and its events (once)
int ensure_comm_stream(bk_ctx *c) {
    CHK(ensure(c->pcnt, 8 * sizeof(unsigned)));
    if (c->cstream) return BK_OK;
    if (!c->hsig) {
        void *hp = nullptr, *dp = nullptr;
        HIPCHK(hipHostMalloc(&hp, 8 * 64, hipHostMallocCoherent));
        memset(hp, 0, 8 * 64);
        const hipError_t e = hipHostGetDevicePointer(&dp, hp, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(hp);
            return fail(BK_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
        }
        c->hsig = (unsigned *)hp;
        c->hsig_d = (unsigned *)dp;
    }

    // normal priority: a highest-priority stream was measured slower in every
    // form (two-digit certified 1.38 -> 1.77 ms, fp32 MFMA 4.39 -> 5.12 ms at
    // E's 8-rank shard)
    hipStream_t cs = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipError_t e = hipSuccess;
    hipEvent_t ev[9] = {};
    for (int i = 0; i < 9 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        (void)hipStreamDestroy(cs);
        return fail(BK_EHIP, "communication stream events: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < 8; ++i) c->ev_piece[i] = ev[i];
    c->ev_cdone = ev[8];
    c->cstream = cs;
    return BK_OK;
}

// The sharded call with its exchange overlapped with the Gram (bk_comm_set_mode
// 2).  ONE Gram launch runs the pieces' workgroups in piece order, each
// workgroup counting itself into its piece's signal word at exit (PieceMarks).
// The communication stream waits for piece p's count (hipStreamWaitValue32),
// reduces piece p's sub-tiles (K1b, or K1i8's reduce of its range) and
// all-reduces them while the Gram's later pieces still run; the last piece is
// reduced on the context stream after the Gram, with the trailing record, and
// all-reduced last.  Every sub-tile is summed from the same partials in the
// same order as the serial path and the all-reduce sums element by element,
// so every output is bitwise that of mode 0.  A failure before the Gram's
// launch is queued poisons the record and joins every piece's all-reduce with
// no wait; the waits are queued only behind a launched Gram, whose every
// workgroup counts itself (idle ones included), so they always resolve.
int sharded_overlapped(bk_ctx *c, const Pieces &pc, const void *dX, int dtype, int64_t n,
                       int64_t dl, int64_t ld, int64_t f, double *U, Plan &pl, int64_t *d_sel,
                       double *d_scores, double *d_mean, const ScoreSplit &sp) {
    const int k = pc.k;
    pl.n = (int)n;
    pl.d = dl;
    pl.T = (int)((n + 63) / 64);
    pl.ntile = pl.T * (pl.T + 1) / 2;
    PieceMarks pm;
    pm.cnt = (unsigned *)c->pcnt.p;
    // r6: the host polls the piece words and queues each piece's reduce and
    // all-reduce as it completes.  A hipStreamWaitValue32 on the communication
    // stream (the probe build's BK_PIECES_DEVWAIT) held a command-processor
    // wait for the whole Gram and slowed it (E's 8-rank shard, exact: +0.85 ms
    // for the wait alone)
    if (probe_env("BK_PIECES_DEVWAIT") && !c->sigcnt[0])
        for (int i = 0; i < 8; ++i) {  // HIP hands signal memory out 8 bytes at a time
            void *sp = nullptr;
            HIPCHK(hipExtMallocWithFlags(&sp, 8, hipMallocSignalMemory));
            c->sigcnt[i] = (unsigned *)sp;
        }
    const bool devwait = probe_env("BK_PIECES_DEVWAIT") != nullptr && c->sigcnt[0];
    for (int p = 0; p < k; ++p) pm.sig[p] = devwait ? c->sigcnt[p] : c->hsig_d + 16 * p;
    if (c->sig_pending) {
        // a previous call's Gram may still store into the words (its host
        // wait was cut short): let it drain before they are reset
        (void)hipStreamSynchronize(c->stream);
        c->sig_pending = false;
    }
    for (int p = 0; p < 8; ++p) __atomic_store_n(c->hsig + 16 * p, 0u, __ATOMIC_RELEASE);
    pm.k = k;
    int tot = 0;
    for (int p = 0; p < k; ++p) {
        pm.start[p] = tot;
        tot += pc.nwg[(size_t)p];
    }
    pm.start[k] = tot;
    bk_ctx::I8Cached *e8 = i8_prepared(c, dX, dtype, n, dl, ld);
    Plan3 *p3 = nullptr;
    double *part = nullptr;
    const bool f32m = f32_mfma_now(c, dtype);
    int st = BK_OK;
    if (!e8) {
        st = get_plan3(c, n, dl, v3_bk(dtype), &p3);
        if (st == BK_OK) st = ensure(c->part, (size_t)p3->nvwg * 16 * 4096 * sizeof(double));
        if (st == BK_OK) part = (double *)c->part.p;
    }
    // 1. zero the piece counts; K1i8: the digit slices; then the one Gram launch
    bool launched = false;
    for (int p = 0; p < k && st == BK_OK && devwait; ++p) {
        const hipError_t e = hipMemsetAsync(c->sigcnt[p], 0, 8, c->stream);
        if (e != hipSuccess) st = fail(BK_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (st == BK_OK) {
        const hipError_t e = hipMemsetAsync(c->pcnt.p, 0, 8 * sizeof(unsigned), c->stream);
        if (e != hipSuccess) st = fail(BK_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (st == BK_OK && c->test_fail_piece)  // test knob BK_TEST_FAIL_PIECE (bk_create)
        st = fail(BK_EHIP, "test knob BK_TEST_FAIL_PIECE=%d: the Gram fails before its launch",
                  c->test_fail_piece);
    if (st == BK_OK && e8)
        st = timed(c, BK_K_SLICE, [&] {
            return launch_i8_slice(dX, dtype, ld, (int)n, dl, e8->L, c->i8ws.p, e8->tables, c->stream);
        });
    // probe build: BK_PIECES_NOMARK=1 -- the pieces' workgroup order with no
    // counts, every piece reduced on the context stream after the Gram (an A/B
    // of the order alone; timing only)
    const bool nomark = probe_env("BK_PIECES_NOMARK") != nullptr;
    if (nomark) pm.k = 0;
    // probe build, timing only (wrong results): BK_PIECES_NOWT=1 -- counts
    // without write-through stores; BK_PIECES_NOCSTREAM=1 -- counts and
    // write-through stores, but the communication stream neither reduces nor
    // all-reduces the early pieces
    if (probe_env("BK_PIECES_NOWT")) pm.nowt = 1;
    const bool nocs = probe_env("BK_PIECES_NOCSTREAM") != nullptr;
    // the communication stream starts behind everything queued before the
    // Gram (the counts' reset, the previous call's finish still reading U) --
    // NOT behind the Gram itself, whose pieces it takes as they complete
    // (r6 fix: this record sat after the Gram launch, so the early pieces'
    // work waited for the whole Gram and nothing overlapped)
    bool cs_started = false;
    if (st == BK_OK && !nomark) {
        HIPCHK(hipEventRecord(c->ev_piece[0], c->stream));
        HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_piece[0], 0));
        cs_started = true;
    }
    if (st == BK_OK) {
        st = timed(c, BK_K_GRAM, [&] {
            return e8 ? launch_i8_gemm((int)n, e8->L, c->i8ws.p, e8->tables, c->stream, pc.d, tot, pm)
                      : launch_gram3(dX, dtype, ld, (int)n, dl, *p3, part, c->stream, c->gram_mode,
                                     nullptr, f32m, pc.d, tot, pm);
        });
        launched = st == BK_OK;
        if (launched && !devwait && !nomark) c->sig_pending = true;
    }
    if (nomark && launched) {
        for (int p = 0; p < k; ++p) {
            const int64_t e0 = pc.e[(size_t)p], e1 = p + 1 == k ? (int64_t)pl.ntile * 4096 : pc.e[(size_t)p + 1];
            HIPCHK(e8 ? launch_i8_reduce(dl, e8->L, c->i8ws.p, U, c->stream, e0, e1, p + 1 == k)
                      : launch_reduce3(part, *p3, U, c->stream, f32m, (int)(e0 / 4096), (int)(e1 / 4096),
                                       p + 1 == k));
        }
        const int64_t usz = bk_upper_elems(n);
        RCCLCHK(ncclAllReduce(U, U, (size_t)usz, ncclDouble, ncclSum, c->comm, c->stream));
        ++c->exchanges;
        return stage_finish(c, U, pl, dX, dtype, n, dl, ld, f, d_sel, d_scores, d_mean, sp);
    }
    const std::string st_msg = st == BK_OK ? std::string() : g_err;
    if (st != BK_OK) CHK(poison_upper(c, U, n));
    if (!cs_started || !launched) {
        // no Gram ran: the communication stream starts behind the poisoned record
        HIPCHK(hipEventRecord(c->ev_piece[0], c->stream));
        HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_piece[0], 0));
    }
    hipEvent_t ar_a = nullptr, ar_b = nullptr, ex_a = nullptr, ex_b = nullptr;
    const bool t_ar = timing_on(c, BK_K_ALLREDUCE), t_ex = timing_on(c, BK_K_EXCHANGE_EXPOSED);
    auto reduce_piece = [&](int p, hipStream_t s, bool rec) -> hipError_t {
        const int64_t e0 = pc.e[(size_t)p], e1 = rec ? (int64_t)pl.ntile * 4096 : pc.e[(size_t)p + 1];
        if (e8) return launch_i8_reduce(dl, e8->L, c->i8ws.p, U, s, e0, e1, rec);
        return launch_reduce3(part, *p3, U, s, f32m, (int)(e0 / 4096), (int)(e1 / 4096), rec);
    };
    // pieces 0 .. k-2 on the communication stream, each as soon as its
    // workgroups are done; the last piece (and the record) on the context
    // stream after the Gram, all-reduced there too once the communication
    // stream's all-reduces are done -- one stream hop at the end, not two
    const bool nowait = probe_env("BK_PIECES_NOWAIT") != nullptr;  // probe: no wait, no early work
    for (int p = 0; p + 1 < k; ++p) {
        // the exchange's span starts when piece 0 is done (after its wait), so
        // span - exposed is the exchange work that ran under the Gram
        auto span_start = [&]() -> int {
            if (p == 0 && t_ar && !ar_a) {
                CHK(get_event(c, &ar_a));
                HIPCHK(hipEventRecord(ar_a, c->cstream));
            }
            return BK_OK;
        };
        if (nowait) {
            CHK(span_start());
            continue;
        }
        if (launched && devwait) {
            HIPCHK(hipStreamWaitValue32(c->cstream, c->sigcnt[p], 1u, hipStreamWaitValueGte,
                                        0xffffffffu));
        } else if (launched) {
            // until the piece's last workgroup stores its word -- or the
            // context stream has drained (the Gram done, or failed), which
            // the stream query below notices
            const volatile unsigned *w = c->hsig + 16 * p;
            for (unsigned spin = 1; __atomic_load_n(w, __ATOMIC_ACQUIRE) == 0u; ++spin) {
                _mm_pause();
                if ((spin & 1023u) == 0u && hipStreamQuery(c->stream) != hipErrorNotReady) break;
            }
            if (p + 2 == k) c->sig_pending = false;  // every word this Gram stores has been seen
        }
        CHK(span_start());
        if (launched) {
            if (nocs) continue;
            HIPCHK(reduce_piece(p, c->cstream, false));
        }
        if (nocs && launched) continue;
        const int64_t e0 = pc.e[(size_t)p], e1 = pc.e[(size_t)p + 1];
        RCCLCHK(ncclAllReduce(U + e0, U + e0, (size_t)(e1 - e0), ncclDouble, ncclSum, c->comm,
                              c->cstream));
    }
    HIPCHK(hipEventRecord(c->ev_cdone, c->cstream));
    if (launched) {
        const hipError_t e = reduce_piece(k - 1, c->stream, true);
        if (e != hipSuccess) {
            CHK(poison_upper(c, U, n));
            st = fail(BK_EHIP, "K1b of the last piece: %s", hipGetErrorString(e));
        }
    }
    if (t_ex) {  // the exposed part: the last piece reduced -> its all-reduce done
        CHK(get_event(c, &ex_a));
        HIPCHK(hipEventRecord(ex_a, c->stream));
    }
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_cdone, 0));
    {
        const int64_t e0 = pc.e[(size_t)k - 1], e1 = pc.e[(size_t)k];
        RCCLCHK(ncclAllReduce(U + e0, U + e0, (size_t)(e1 - e0), ncclDouble, ncclSum, c->comm,
                              c->stream));
    }
    if (t_ar) {  // the span: the first all-reduce's start -> the last one's end
        CHK(get_event(c, &ar_b));
        HIPCHK(hipEventRecord(ar_b, c->stream));
        c->pending.push_back({BK_K_ALLREDUCE, ar_a, ar_b});
    }
    if (t_ex) {
        CHK(get_event(c, &ex_b));
        HIPCHK(hipEventRecord(ex_b, c->stream));
        c->pending.push_back({BK_K_EXCHANGE_EXPOSED, ex_a, ex_b});
    }
    c->exchanged_bytes += (double)bk_upper_elems(n) * sizeof(double);
    ++c->exchanges;
    if (st != BK_OK) {
        (void)stage_finish(c, U, pl, dX, dtype, n, dl, ld, f, d_sel, d_scores, nullptr, sp);
        g_err = st_msg.empty() ? g_err : st_msg;
        return st;
    }
    return stage_finish(c, U, pl, dX, dtype, n, dl, ld, f, d_sel, d_scores, d_mean, sp);
}

// one pass of the sharded entry: partial Gram of the local columns (zeros for
// an empty shard), the exchange, then scores/selection and the local mean.
//
// No rank may leave its peers inside the collective.  Everything that can fail
// before it is an allocation (U, the all-gather buffer, K1's plan and slabs)
// or a launch.  On the first call of a signature (n, f, dtype, exchange mode),
// which every rank makes together, the workspace is allocated and the ranks
// all-reduce (max) a status word before the exchange, so an allocation
// failure on one rank is an error on every rank (BK_ERCCL on the others).
// Later calls of the same signature allocate nothing that depends on the rank
// alone but K1's slabs for a changed d_local; any failure there (or a failed
// launch) poisons the rank's partial (NaN trailing pair) and the rank still
// joins the exchange, so every rank's finish marks the call invalid
// (MARGIN_POISONED) and the failing rank returns its own error.
int sharded_once(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t dl, int64_t ld,
                 int64_t f, int64_t *d_sel, double *d_scores, double *d_mean) {
    const int64_t usz = bk_upper_elems(n);
    const bool exch = c->comm != nullptr;
    // the call's signature, the same on every rank by the API's contract: a
    // change makes the ranks agree again (status, and the overlapped piece layout)
    const int sig = c->deterministic + 2 * c->overlap +
                    32 * (dtype == BK_F32 ? c->f32_mode : c->f64_mode);
    const bool agree = exch && (c->nranks > 1 || c->test_fail_exchange) &&
                       (n != c->agreed_n || f != c->agreed_f || dtype != c->agreed_dtype ||
                        sig != c->agreed_det);
    const ScoreSplit sp = score_split(c, n);
    int prep = ensure(c->U, (size_t)usz * sizeof(double));
    if (prep == BK_OK && exch && c->deterministic)
        prep = ensure(c->Ug, (size_t)usz * c->nranks * sizeof(double));
    if (prep == BK_OK && sp.parts > 1) prep = prepare_finish(c, n, sp, d_scores == nullptr);
    if (prep == BK_OK && dl > 0) prep = prepare_gram(c, dX, dtype, n, dl, ld);
    // bk_comm_set_mode 2: the Gram in pieces, each all-reduced on the
    // communication stream while the next computes (nullptr: this call's
    // Gram has no such split -- it is computed whole and exchanged after)
    const Pieces *pcs = nullptr;
    if (prep == BK_OK && exch && c->overlap >= 2 && !c->deterministic && dl > 0) {
        if (c->wait_value_ok < 0) {
            int v = 0;
            c->wait_value_ok = hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue,
                                                     c->device) == hipSuccess && v ? 1 : 0;
            (void)hipGetLastError();
        }
        if (c->wait_value_ok) {
            prep = gram_pieces(c, dX, dtype, n, dl, ld, c->overlap, &pcs);
            if (prep == BK_OK && pcs) prep = ensure_comm_stream(c);
        }
    }
    if (prep == BK_OK && c->test_fail_exchange == (agree ? 1 : 2))
        prep = fail(BK_ENOMEM, "test knob BK_TEST_FAIL_BEFORE_EXCHANGE=%d: forced failure",
                    c->test_fail_exchange);
    const std::string prep_msg = prep == BK_OK ? std::string() : g_err;
    if (agree) {
        // one max-all-reduce of {status, piece layout, -piece layout}: the ranks
        // learn whether any failed, and whether they all cut the Gram into the
        // same pieces (the layout's fingerprint equal on every rank: max ==
        // -max(-fp)).  A rank whose plan does not split, or a different cut,
        // turns the overlapped exchange off on every rank for this signature:
        // each piece is one collective, so the ranks must agree on them.
        double *w = (double *)c->status.p;
        double v[3] = {prep == BK_OK ? 0.0 : 1.0, 0.0, 0.0};
        if (pcs) {
            uint64_t h = 1469598103934665603ull;
            auto mix = [&](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
            mix((uint64_t)pcs->k);
            for (int64_t x : pcs->e) mix((uint64_t)x);
            v[1] = (double)(h >> 12) + 1.0;  // 52 bits: exact in a double, never 0
        }
        v[2] = -v[1] - (c->test_pieces_disagree ? 1.0 : 0.0);
        HIPCHK(hipMemcpyAsync(w, v, sizeof v, hipMemcpyHostToDevice, c->stream));
        RCCLCHK(ncclAllReduce(w, w, 3, ncclDouble, ncclMax, c->comm, c->stream));
        HIPCHK(hipMemcpyAsync(v, w, sizeof v, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const double any = v[0];
        c->overlap_agreed = v[1] != 0.0 && v[1] == -v[2];
        if (prep != BK_OK) {
            g_err = prep_msg;
            return prep;
        }
        if (any != 0.0)
            return fail(BK_ERCCL, "a peer rank failed before the Gram exchange (status agreement "
                                  "of the call's first signature); no exchange was made");
        c->agreed_n = n;
        c->agreed_f = f;
        c->agreed_dtype = dtype;
        c->agreed_det = sig;
    } else if (prep != BK_OK && (!exch || c->U.bytes < (size_t)usz * sizeof(double))) {
        return prep;  // nothing to join (no communicator), or no partial to poison
    }
    double *U = (double *)c->U.p;
    Plan pl;
    pl.n = (int)n;
    pl.T = (int)((n + 63) / 64);
    pl.ntile = pl.T * (pl.T + 1) / 2;
    int st = prep;
    if (!c->overlap_agreed) pcs = nullptr;  // a peer cut the Gram differently (or not at all)
    if (pcs && st == BK_OK)
        return sharded_overlapped(c, *pcs, dX, dtype, n, dl, ld, f, U, pl, d_sel, d_scores, d_mean,
                                  sp);
    if (st == BK_OK) {
        if (dl > 0) {
            st = stage_gram(c, dX, dtype, n, dl, ld, U, pl);
        } else {
            // an empty column shard (d small against the rank count): a zero
            // partial (column counts 0 too), so this rank still joins the exchange
            const hipError_t e = hipMemsetAsync(U, 0, (size_t)usz * sizeof(double), c->stream);
            if (e != hipSuccess) st = fail(BK_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        }
    }
    const std::string st_msg = st == BK_OK ? std::string() : g_err;
    if (st != BK_OK) CHK(poison_upper(c, U, n));
    if (exch) {  // also at 1 rank, so the exchange is exercised on a 1-GPU box
        hipEvent_t a = nullptr, b = nullptr;
        const bool ton = timing_on(c, BK_K_ALLREDUCE);
        if (ton) {
            CHK(get_event(c, &a));
            CHK(get_event(c, &b));
            HIPCHK(hipEventRecord(a, c->stream));
        }
        if (!c->deterministic) {
            RCCLCHK(ncclAllReduce(U, U, (size_t)usz, ncclDouble, ncclSum, c->comm, c->stream));
        } else {
            double *Ug = (double *)c->Ug.p;
            RCCLCHK(ncclAllGather(U, Ug, (size_t)usz, ncclDouble, c->comm, c->stream));
            HIPCHK(launch_sum_ranks(Ug, c->nranks, usz, U, c->stream));
        }
        if (ton) {
            HIPCHK(hipEventRecord(b, c->stream));
            c->pending.push_back({BK_K_ALLREDUCE, a, b});
        }
        c->exchanged_bytes += (double)usz * sizeof(double) * (c->deterministic ? c->nranks : 1);
        ++c->exchanges;
    }
    if (st != BK_OK) {
        // the rest of the finish still runs, so this rank's record says so too
        (void)stage_finish(c, U, pl, dX, dtype, n, dl, ld, f, d_sel, d_scores, nullptr, sp);
        g_err = st_msg;
        return st;
    }
    return stage_finish(c, U, pl, dX, dtype, n, dl, ld, f, d_sel, d_scores,
                        dl > 0 ? d_mean : nullptr, sp);
}
}  // namespace

int bk_multikrum_sharded_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t dl,
                                int64_t ld, int64_t f, int64_t *d_sel, double *d_scores,
                                double *d_mean) {
    if (dl > 0) {
        CHK(check_common(c, dX, dtype, n, dl, ld));
    } else {
        // d_local = 0 is legal (an empty trailing shard): dX, ld and d_mean are unused
        if (!c) return fail(BK_EINVAL, "null context");
        if (dl < 0) return fail(BK_EINVAL, "d_local=%lld < 0", (long long)dl);
        if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype %d", dtype);
    }
    CHK(bk_check_args(n, dl > 0 ? dl : 1, f));
    if (!d_sel) return fail(BK_EINVAL, "null d_sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (c->nranks > 1 && !c->comm) return fail(BK_ERCCL, "bk_comm_init not called");
    auto once = [&] { return sharded_once(c, dX, dtype, n, dl, ld, f, d_sel, d_scores, d_mean); };
    if (certified(c, dtype)) return run_certified(c, once);
    return once();
}

int bk_comm_size(bk_ctx *c, int *nranks, int *rank) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    int nr = 1, rk = 0;
    if (c->comm) {
        RCCLCHK(ncclCommCount(c->comm, &nr));
        RCCLCHK(ncclCommUserRank(c->comm, &rk));
    }
    if (nranks) *nranks = c->comm ? nr : 0;
    if (rank) *rank = rk;
    return BK_OK;
}

int bk_comm_stats(bk_ctx *c, int64_t *exchanges, double *bytes) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (exchanges) *exchanges = c->exchanges;
    if (bytes) *bytes = c->exchanged_bytes;
    return BK_OK;
}

}  // extern "C"
