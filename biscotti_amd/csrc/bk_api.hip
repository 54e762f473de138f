// bk_api.hip -- the C ABI (include/bk.h): the error string, the context and its
// workspace basics, streams, plans and modes, the device-resident entries and
// the hipGraph replay, the margin readers, per-kernel HIP-event timing.  No
// torch, no C++ types across the boundary; every failure becomes a negative
// status + bk_last_error().  The other entry families: bk_stage.hip (K1..K4
// staging), bk_host.hip, bk_comm.hip, bk_group.hip, bk_entries.hip,
// bk_collect.hip; bk_ctx.h is what they share.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "bk_ctx.h"
#include "bk_hostpool.h"
#include "bk_synth.h"

namespace bk {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char *kKernelNames[BK_NUM_KERNELS] = {"k_gram",    "k_reduce",  "k_transpose", "k_scores",
                                            "k_rank",    "k_compact", "k_mean",   "allreduce",
                                            "k_synth",   "h2d",       "d2h",
                                            "k_aggregate", "k_qsum",  "k_noise",
                                            "k_roni", "k_small", "k_slice", "score_gather",
                                            "exchange_exposed", "k_roni_round", "k_roni_round_sm"};

int ensure(DevBuf &b, size_t bytes) {
    if (bytes <= b.bytes) return BK_OK;
    if (b.epoch) ++*b.epoch;  // pointers baked into captured graphs are about to change
    if (b.p) {
        hipError_t e = hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
        if (e != hipSuccess) return fail(BK_EHIP, "hipFree: %s", hipGetErrorString(e));
    }
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(BK_ENOMEM, "hipMalloc(%zu bytes): %s", want, hipGetErrorString(e));
    }
    b.bytes = want;
    return BK_OK;
}

int get_event(bk_ctx *c, hipEvent_t *out) {
    if (!c->pool.empty()) {
        *out = c->pool.back();
        c->pool.pop_back();
        return BK_OK;
    }
    HIPCHK(hipEventCreate(out));
    return BK_OK;
}

// Bracket one launch with events when timing is on.
bool timing_on(bk_ctx *c, int kid) {
    if (!((c->timing >> kid) & 1u)) return false;
    return c->tstride <= 1 || (c->tseq[kid]++ % c->tstride) == 0;
}

int check_common(bk_ctx *c, const void *X, int dtype, int64_t n, int64_t d, int64_t ld) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!X) return fail(BK_EINVAL, "null X");
    if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype %d", dtype);
    if (n < 1 || d < 1) return fail(BK_EINVAL, "need n >= 1 and d >= 1 (n=%lld d=%lld)",
                                   (long long)n, (long long)d);
    if (n > BK_MAX_N) return fail(BK_ENOTSUP, "n=%lld exceeds BK_MAX_N=%d", (long long)n, BK_MAX_N);
    if (ld < d) return fail(BK_EINVAL, "ld=%lld < d=%lld", (long long)ld, (long long)d);
    return BK_OK;
}

size_t esize(int dtype) { return dtype == BK_F64 ? 8 : 4; }

bool certified(const bk_ctx *c, int dtype) {
    if (dtype == BK_F64) return c->f64_mode == BK_F64_I8_CERTIFIED || c->f64_mode == BK_F64_I8X2_CERTIFIED;
    return c->f32_mode == BK_F32_CERTIFIED || c->f32_mode == BK_F32_I8_CERTIFIED ||
           c->f32_mode == BK_F32_I8X2_CERTIFIED;
}

}  // namespace bk

namespace {

void drop_graph(bk_ctx::CachedGraph &cg) {
    if (cg.exec) (void)hipGraphExecDestroy(cg.exec);
    if (cg.g) (void)hipGraphDestroy(cg.g);
    cg.exec = nullptr;
    cg.g = nullptr;
}

// every workspace buffer of c bumps c->ws_epoch when it is reallocated
void bind_epoch(bk_ctx *c) {
    DevBuf *bufs[] = {&c->part, &c->U,    &c->Ug,   &c->scores, &c->mask,   &c->sel,
                      &c->X,    &c->mean, &c->perm, &c->trace,  &c->idx,    &c->roni_X,
                      &c->roni_y, &c->roni_w, &c->roni_d, &c->roni_cnt, &c->roni_s,
                      &c->noise, &c->diag, &c->bnd, &c->Ut, &c->small_ctr, &c->small_part,
                      &c->mean_part, &c->status, &c->rmc_X, &c->rmc_y, &c->rmc_ws,
                      &c->rmc_xn, &c->rmc_idx, &c->rmc_nt, &c->i8ws, &c->sgather, &c->pcnt};
    for (DevBuf *b : bufs) b->epoch = &c->ws_epoch;
}

}  // namespace

extern "C" {

int bk_abi_version(void) { return BK_ABI_VERSION; }

const char *bk_last_error(void) { return g_err.c_str(); }

int bk_check_args(int64_t n, int64_t d, int64_t f) {
    if (n < 1 || d < 1) return fail(BK_EINVAL, "need n >= 1 and d >= 1");
    if (f < 1 || f >= n)
        return fail(BK_EINVAL, "need 1 <= f < n (n=%lld f=%lld); f=0 is the reference's "
                               "argpartition ValueError",
                    (long long)n, (long long)f);
    if (n > BK_MAX_N) return fail(BK_ENOTSUP, "n=%lld exceeds BK_MAX_N=%d", (long long)n, BK_MAX_N);
    return BK_OK;
}

const char *bk_kernel_name(int kid) {
    return (kid >= 0 && kid < BK_NUM_KERNELS) ? kKernelNames[kid] : "?";
}

int64_t bk_upper_elems(int64_t n) {
    const int64_t T = (n + 63) / 64;
    // + the trailing record {column count, columns on the fp32 MFMA, the int8
    // Gram's absolute error bound, 0} (K3b's margin; summed by every exchange)
    return T * (T + 1) / 2 * 4096 + BK_UPPER_TRAIL;
}

int bk_create(bk_ctx **out, int device) {
    if (!out) return fail(BK_EINVAL, "null out");
    *out = nullptr;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(BK_EINVAL, "device %d out of range (%d visible)", device, ndev);
    bk_ctx *c = new (std::nothrow) bk_ctx();
    if (!c) return fail(BK_ENOMEM, "host allocation of bk_ctx failed");
    c->device = device;
    bind_epoch(c);
    DeviceGuard dg(device);
    // probe knob: how the host waits for the GPU (hipDeviceScheduleSpin 1,
    // Yield 2, BlockingSync 4; tools/idle_probe.py)
    if (const char *v = probe_env("BK_SCHED")) (void)hipSetDeviceFlags((unsigned)atoi(v));
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) c->num_cu = prop.multiProcessorCount;
    e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(BK_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->stream = c->own;
    if (const char *v = probe_env("BK_GRAM"))
        if (strcmp(v, "v1") == 0) c->gram_variant = 1;
    if (const char *v = probe_env("BK_GRAM_MODE")) c->gram_mode = atoi(v);
    if (const char *v = getenv("BK_SMALL")) c->small_on = atoi(v) != 0;
    if (const char *v = getenv("BK_SPIN_US")) c->spin_us = atoll(v);
    // test / debug knobs (tests/test_gpu_errors.py): a hand-off wait that gives
    // up after this many polls; the queue-line invariant check; a sharded call
    // that fails before its exchange
    if (const char *v = getenv("BK_SMALL_SPIN_MAX")) {
        char *end = nullptr;
        c->small_spin_max = strtoull(v, &end, 10);
        if (end && *end == ',') c->small_spin_left = strtoll(end + 1, nullptr, 10);
    }
    if (const char *v = getenv("BK_SMALL_CHECK_LINES")) c->small_check_lines = atoi(v) != 0;
    if (const char *v = getenv("BK_TEST_FAIL_BEFORE_EXCHANGE")) c->test_fail_exchange = atoi(v);
    if (const char *v = getenv("BK_TEST_I8_ENOMEM")) c->test_i8_enomem = atoi(v) != 0;
    if (const char *v = getenv("BK_TEST_FAIL_PIECE")) c->test_fail_piece = atoi(v);
    if (const char *v = getenv("BK_TEST_PIECES_DISAGREE")) c->test_pieces_disagree = atoi(v);
    if (const char *v = getenv("BK_SPLIT_SCORES_MIN_N")) c->split_min_n = atoll(v);
    if (const char *v = getenv("BK_TEST_SPLIT_SCORES")) c->test_split_scores = atoi(v);
    if (const char *v = getenv("BK_EMU_SPLIT_SCORES")) c->emu_split_scores = atoi(v);
    if (const char *v = getenv("BK_TEST_SPLIT_FAIL")) c->test_split_fail = atoi(v);
    // the block's path cuts in bytes (bk_ctx.h BLOCK_*_MAX; tools/block_bench.py
    // and the tests of both sides of a cut), capped at what the arrival block holds
    const auto cut = [](const char *name, int64_t &out, int64_t cap) {
        if (const char *v = getenv(name)) {
            const int64_t x = atoll(v);
            out = x < 0 ? 0 : x > cap ? cap : x;
        }
    };
    cut("BK_BLOCK_MAPPED_HOST", c->block_mapped_host, 4 << 20);
    cut("BK_BLOCK_MAPPED_PINNED", c->block_mapped_pinned, 4 << 20);
    cut("BK_BLOCK_FIN", c->block_fin_max, INT64_MAX);
    // bk_block_finish_eval's two routes, bit-identical (tools/eval_bench.py)
    // (1: the sequence everywhere, 0: one wait everywhere; unset: routed)
    if (const char *v = getenv("BK_BLOCK_EVAL_SEQ")) c->block_eval_one_wait = atoi(v) ? 0 : 2;
    if (const char *v = getenv("BK_SHARES_GEN_PER_CHUNK")) c->shares_gen_per_chunk = atoi(v) ? 1 : 0;
    e = configure_kernels();
    if (e == hipSuccess) e = configure_aggregate_kernels();
    if (e == hipSuccess) e = configure_i8_kernels();
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->own);
        delete c;
        return fail(BK_EHIP, "configure_kernels: %s", hipGetErrorString(e));
    }
    *out = c;
    return BK_OK;
}

void bk_destroy(bk_ctx *c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceGuard dg(c->device);
        (void)hipStreamSynchronize(c->stream);
        DevBuf *bufs[] = {&c->part, &c->U,    &c->Ug,  &c->scores,
                          &c->mask, &c->sel,  &c->X,   &c->mean, &c->perm, &c->trace, &c->idx,
                          &c->roni_X, &c->roni_y, &c->roni_w, &c->roni_d, &c->roni_cnt, &c->roni_s,
                          &c->noise, &c->diag, &c->bnd, &c->Ut, &c->small_ctr, &c->small_part,
                          &c->mean_part, &c->status, &c->rmc_X, &c->rmc_y, &c->rmc_ws,
                      &c->rmc_xn, &c->rmc_idx, &c->rmc_nt, &c->i8ws, &c->sgather, &c->pcnt,
                          &c->rr_w, &c->rr_base, &c->rr_ws, &c->rs_w, &c->rs_base, &c->rs_ws,
                          &c->round_rows, &c->round_cnt, &c->round_idx,
                          &c->batch_ctr, &c->batch_part, &c->batch_diag, &c->batch_scores,
                          &c->batch_rec, &c->batch_X, &c->batch_sel, &c->batch_hsc, &c->batch_mean,
                          &c->batch_desc};
        if (c->hmargin) (void)hipHostFree(c->hmargin);
        if (c->hout) (void)hipHostFree(c->hout);
        if (c->round_out) (void)hipHostFree(c->round_out);
        if (c->ev_round) (void)hipEventDestroy(c->ev_round);
        for (void *p : c->ragged_stage)
            if (p) (void)hipHostFree(p);
        for (hipEvent_t ev : c->ev_ragged)
            if (ev) (void)hipEventDestroy(ev);
        if (c->copy) (void)hipStreamSynchronize(c->copy);
        for (DevBuf *b : bufs)
            if (b->p) (void)hipFree(b->p);
        for (hipEvent_t ev : {c->ev_go, c->ev_cp[0], c->ev_cp[1], c->ev_use[0], c->ev_use[1],
                              c->ev_rows[0], c->ev_rows[1], c->ev_rows[2], c->ev_rows[3]})
            if (ev) (void)hipEventDestroy(ev);
        if (c->cstream) (void)hipStreamSynchronize(c->cstream);
        for (hipEvent_t ev : c->ev_piece)
            if (ev) (void)hipEventDestroy(ev);
        if (c->ev_cdone) (void)hipEventDestroy(c->ev_cdone);
        if (c->cstream) (void)hipStreamDestroy(c->cstream);
        for (unsigned *sgc : c->sigcnt)
            if (sgc) (void)hipFree(sgc);
        if (c->hsig) (void)hipHostFree(c->hsig);
        if (c->rstage) (void)hipHostFree(c->rstage);
        collect_destroy(c->collect);
        block_destroy(c->block);
        eval_destroy(c->eval);
        shares_destroy(c->shares);
        grad_destroy(c->grad);
        commit_destroy(c->commit);
        delete c->hpool;
        if (c->copy) (void)hipStreamDestroy(c->copy);
        for (void *p : c->staged) (void)hipHostFree(p);
        for (auto &ev : c->pending) {
            (void)hipEventDestroy(ev.a);
            (void)hipEventDestroy(ev.b);
        }
        for (hipEvent_t ev : c->pool) (void)hipEventDestroy(ev);
        for (auto &cp : c->plans) {
            free_plan(cp.p);
            free_pieces(cp.pc);
        }
        for (auto &e : c->i8) {
            if (e.tables) (void)hipFree(e.tables);
            free_pieces(e.pc);
        }
        for (auto &cg : c->graphs) drop_graph(cg);
        if (c->comm) (void)ncclCommDestroy(c->comm);
        if (c->own) (void)hipStreamDestroy(c->own);
    }
    delete c;
}

int bk_set_stream(bk_ctx *c, void *s) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->stream = s ? (hipStream_t)s : c->own;
    return BK_OK;
}

void *bk_get_stream(bk_ctx *c) { return c ? (void *)c->stream : nullptr; }

int bk_synchronize(bk_ctx *c) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    HIPCHK(wait_stream(c));
    if (c->margin_unchecked) {  // the last finish's error codes (an asynchronous caller's only check)
        double mg[MARGIN_WORDS];
        CHK(read_margin(c, mg));
    }
    return BK_OK;
}

int bk_stage_alloc(bk_ctx *c, int64_t bytes, void **pinned) {
    if (!c || !pinned || bytes <= 0) return fail(BK_EINVAL, "bad stage_alloc arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable);
    if (e != hipSuccess) return fail(BK_ENOMEM, "hipHostMalloc(%lld): %s", (long long)bytes,
                                     hipGetErrorString(e));
    c->staged.push_back(p);
    *pinned = p;
    return BK_OK;
}

int bk_stage_free(bk_ctx *c, void *p) {
    if (!c || !p) return fail(BK_EINVAL, "bad stage_free arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    for (size_t i = 0; i < c->staged.size(); ++i) {
        if (c->staged[i] == p) {
            c->staged.erase(c->staged.begin() + i);
            HIPCHK(hipHostFree(p));
            return BK_OK;
        }
    }
    return fail(BK_EINVAL, "pointer was not allocated by bk_stage_alloc");
}

int bk_plan(bk_ctx *c, int64_t n, int64_t d, int64_t *S, int64_t *kc, int64_t *ntile,
            int64_t *nwg) {
    if (n < 1 || d < 1) return fail(BK_EINVAL, "need n, d >= 1");
    if (n > BK_MAX_N) return fail(BK_ENOTSUP, "n=%lld exceeds BK_MAX_N=%d", (long long)n, BK_MAX_N);
    // the K1 v3 plan for aligned fp64 rows (host tables only, nothing allocated)
    const Plan3Host H = build_plan3((int)n, d, c ? c->num_cu : 256, G3_BK);
    for (int u = 0; u < H.ntile; ++u)
        if (H.red[3 * u + 1] < 0) return fail(BK_EHIP, "internal: K1 plan fails its coverage check");
    if (S) *S = (int64_t)H.groups.size();
    if (kc) *kc = G3_BK;
    if (ntile) *ntile = H.ntile;
    if (nwg) *nwg = (int64_t)(H.seg.size() / 2);
    return BK_OK;
}

int bk_plan_mode(bk_ctx *c, int64_t n, int64_t d, int mode, int rounds, int64_t *S, int64_t *nwg) {
    if (n < 1 || d < 1) return fail(BK_EINVAL, "need n, d >= 1");
    if (n > BK_MAX_N) return fail(BK_ENOTSUP, "n=%lld exceeds BK_MAX_N=%d", (long long)n, BK_MAX_N);
    if (mode < -1 || mode > 3 || rounds < 0 || rounds > 16)
        return fail(BK_EINVAL, "bad planner mode %d / rounds %d", mode, rounds);
    const Plan3Host H = build_plan3((int)n, d, c ? c->num_cu : 256, G3_BK, mode, rounds);
    for (int u = 0; u < H.ntile; ++u)
        if (H.red[3 * u + 1] < 0) return fail(BK_EHIP, "internal: K1 plan fails its coverage check");
    if (S) *S = (int64_t)H.groups.size();
    if (nwg) *nwg = (int64_t)(H.seg.size() / 2);
    return BK_OK;
}

namespace {

// The 7-launch step (K1, K1b, K2, K3, K3b, K4) replayed as one hipGraph: the
// first call of a signature runs eagerly (allocating workspace and the K1
// plan), the second captures the same sequence, later ones replay it.  Only
// without per-kernel timing (events are not captured).
int run_device_graph(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                     int64_t f, int64_t *d_sel, double *d_scores, double *d_mean) {
    for (size_t i = 0; i < c->graphs.size();) {  // retire graphs over stale workspace
        if (c->graphs[i].epoch != c->ws_epoch) {
            drop_graph(c->graphs[i]);
            c->graphs.erase(c->graphs.begin() + i);
        } else {
            ++i;
        }
    }
    for (auto &cg : c->graphs)
        if (cg.X == dX && cg.dtype == dtype && cg.n == n && cg.d == d && cg.ld == ld && cg.f == f &&
            cg.sel == d_sel && cg.scores == d_scores && cg.mean == d_mean) {
            HIPCHK(hipGraphLaunch(cg.exec, c->stream));
            // the captured finish (K3b / k_small) writes the context's record:
            // point the readers at it and arm bk_synchronize's check
            c->margin_valid = 1;
            c->margin_host = c->hmargin;
            c->margin_unchecked = 1;
            return BK_OK;
        }
    // eager run first: every ensure() / plan build happens outside the capture
    const uint64_t e0 = c->ws_epoch;
    CHK(run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean));
    if (c->ws_epoch != e0) return BK_OK;  // workspace moved: capture on the next call
    bk_ctx::CachedGraph cg{dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean, c->ws_epoch, nullptr,
                           nullptr};
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const int st = run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(c->stream, &g);
    if (st != BK_OK) {
        if (g) (void)hipGraphDestroy(g);
        return st;
    }
    if (ee != hipSuccess) return fail(BK_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(ee));
    cg.g = g;
    const hipError_t ei = hipGraphInstantiate(&cg.exec, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) {
        drop_graph(cg);
        return fail(BK_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(ei));
    }
    if (c->ws_epoch != e0) {  // cannot happen after an eager run of the same call; be safe
        drop_graph(cg);
        return BK_OK;
    }
    if (c->graphs.size() >= 4) {
        drop_graph(c->graphs.front());
        c->graphs.erase(c->graphs.begin());
    }
    c->graphs.push_back(cg);
    return BK_OK;  // the captured run is not executed: the eager one produced this call's outputs
}
}  // namespace

int bk_multikrum_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                        int64_t f, int64_t *d_sel, double *d_scores, double *d_mean) {
    CHK(check_common(c, dX, dtype, n, d, ld));
    CHK(bk_check_args(n, d, f));
    if (!d_sel) return fail(BK_EINVAL, "null d_sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (certified(c, dtype))
        return run_certified(c, [&] { return run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean); });
    // (the debug traces synchronize mid-call, which a stream capture refuses)
    if (c->graph_on && c->timing == 0 && !probe_env("BK_TRACE_FILE") && !probe_env("BK_SMALL_TRACE"))
        return run_device_graph(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
    return run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
}

int bk_set_f32_mode(bk_ctx *c, int mode) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (mode < BK_F32_EXACT || mode > BK_F32_I8X2_CERTIFIED)
        return fail(BK_EINVAL, "bad f32 mode %d", mode);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->f32_mode != mode) ++c->ws_epoch;  // captured graphs baked the other kernel in
    c->f32_mode = mode;
    c->i8_failed.clear();  // a new mode tries K1i8's workspace again
    c->emu_split_n = -1;  // BK_EMU_SPLIT_SCORES: the new mode's first call scores every share
    return BK_OK;
}

int bk_set_f64_mode(bk_ctx *c, int mode) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (mode != BK_F64_EXACT && mode != BK_F64_I8 && mode != BK_F64_I8_CERTIFIED &&
        mode != BK_F64_I8X2 && mode != BK_F64_I8X2_CERTIFIED)
        return fail(BK_EINVAL, "bad f64 mode %d", mode);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->f64_mode != mode) ++c->ws_epoch;  // captured graphs baked the other kernel in
    c->f64_mode = mode;
    c->i8_failed.clear();
    c->emu_split_n = -1;
    return BK_OK;
}

int bk_graph_enable(bk_ctx *c, int on) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    c->graph_on = on ? 1 : 0;
    if (!on) {
        for (auto &cg : c->graphs) drop_graph(cg);
        c->graphs.clear();
    }
    return BK_OK;
}

int bk_gram_upper_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                         double *d_upper) {
    CHK(check_common(c, dX, dtype, n, d, ld));
    if (!d_upper) return fail(BK_EINVAL, "null d_upper");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    Plan pl;
    int st = c->test_fail_exchange == 2
                 ? fail(BK_EHIP, "test knob BK_TEST_FAIL_BEFORE_EXCHANGE=2: forced failure")
                 : stage_gram(c, dX, dtype, n, d, ld, d_upper, pl);
    if (st != BK_OK) {
        // a caller that exchanges the partial anyway (so its peers are not left
        // in the collective) hands every rank an invalid record, not a wrong Gram
        const std::string msg = g_err;
        (void)poison_upper(c, d_upper, n);
        g_err = msg;
    }
    return st;
}

int bk_finish_device(bk_ctx *c, const double *d_upper, const void *dX, int dtype, int64_t n,
                     int64_t d, int64_t ld, int64_t f, int64_t *d_sel, double *d_scores,
                     double *d_mean) {
    if (d_mean) CHK(check_common(c, dX, dtype, n, d, ld));
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(bk_check_args(n, d < 1 ? 1 : d, f));
    if (!d_upper || !d_sel) return fail(BK_EINVAL, "null d_upper / d_sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    Plan pl;
    pl.n = (int)n;
    pl.T = (int)((n + 63) / 64);
    pl.ntile = pl.T * (pl.T + 1) / 2;
    return stage_finish(c, d_upper, pl, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
}

int bk_selection_margin(bk_ctx *c, double *gap, double *err_bound, int *near_tie) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    double mg[MARGIN_WORDS];
    CHK(read_margin(c, mg));
    if (gap) *gap = mg[0];
    if (err_bound) *err_bound = mg[1];
    if (near_tie) *near_tie = mg[2] != 0.0 ? 1 : 0;
    return BK_OK;
}

int bk_selection_margin_record(bk_ctx *c, double *record) {
    if (!c || !record) return fail(BK_EINVAL, "null context / record");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    double mg[MARGIN_WORDS];
    CHK(read_margin(c, mg));
    memcpy(record, mg, 8 * sizeof(double));  // the public record (u_G stays internal)
    return BK_OK;
}

int64_t bk_certified_reruns(bk_ctx *c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->certified_reruns;
}

int bk_set_small_path(bk_ctx *c, int on) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->small_on != (on ? 1 : 0)) ++c->ws_epoch;  // captured graphs baked the other path in
    c->small_on = on ? 1 : 0;
    return BK_OK;
}

// (collection finishes are never captured in a graph: no epoch to bump)
int bk_set_collect_wide(bk_ctx *c, int on) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->collect_wide = on ? 1 : 0;
    return BK_OK;
}

int bk_set_collect_wide_arrive(bk_ctx *c, int on) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->collect_wide_arrive = on == 2 ? 2 : on ? 1 : 0;  // 2: every shape of the range
    return BK_OK;
}

int bk_set_collect_tiny(bk_ctx *c, int on) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->collect_tiny = on ? 1 : 0;
    return BK_OK;
}

int bk_synth_fill_device(bk_ctx *c, void *dX, int dtype, int64_t n, int64_t dl, int64_t ld,
                         int64_t c0, int64_t d_total, uint64_t seed, int64_t nbyz, double mu_scale,
                         double byz_scale, double sigma, int flags) {
    CHK(check_common(c, dX, dtype, n, dl, ld));
    if (c0 < 0 || c0 + dl > d_total || nbyz < 0 || nbyz > n)
        return fail(BK_EINVAL, "bad synth column range / nbyz");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    // Fisher-Yates on the host (sequential by definition), then upload
    std::vector<int64_t> perm((size_t)n);
    const uint64_t b3 = stream_base(seed, 3);
    for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
    for (int64_t i = n - 1; i >= 1; --i) {
        const int64_t j = (int64_t)(sm64(b3 + (uint64_t)i) % (uint64_t)(i + 1));
        const int64_t t = perm[(size_t)i];
        perm[(size_t)i] = perm[(size_t)j];
        perm[(size_t)j] = t;
    }
    CHK(ensure(c->perm, (size_t)n * sizeof(int64_t)));
    HIPCHK(hipMemcpyAsync(c->perm.p, perm.data(), (size_t)n * sizeof(int64_t),
                          hipMemcpyHostToDevice, c->stream));
    SynthParams P;
    P.b0 = stream_base(seed, 0);
    P.b1 = stream_base(seed, 1);
    P.b2 = stream_base(seed, 2);
    P.b4 = stream_base(seed, 4);
    P.n = n;
    P.nbyz = nbyz;
    P.d_total = d_total;
    P.mu_scale = mu_scale;
    P.byz_scale = byz_scale;
    P.sigma = sigma;
    P.flags = flags;
    const int64_t *dperm = (const int64_t *)c->perm.p;
    CHK(timed(c, BK_K_SYNTH,
              [&] { return launch_synth(dX, dtype, ld, n, dl, c0, dperm, P, c->stream); }));
    // the host perm vector dies here: make sure the (pageable) copy has landed
    HIPCHK(hipStreamSynchronize(c->stream));
    return BK_OK;
}

int bk_timing_enable(bk_ctx *c, int on) {
    return bk_timing_select(c, on ? ~0u : 0u);
}

namespace {
// drop the accumulated timings and pending events (under c->mu)
int timing_reset(bk_ctx *c) {
    DeviceGuard dg(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &ev : c->pending) {
        c->pool.push_back(ev.a);
        c->pool.push_back(ev.b);
    }
    c->pending.clear();
    for (int i = 0; i < BK_NUM_KERNELS; ++i) {
        c->tot_ms[i] = 0;
        c->cnt[i] = 0;
        c->tseq[i] = 0;
    }
    return BK_OK;
}
}  // namespace

int bk_timing_stride(bk_ctx *c, int every) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (every < 1) return fail(BK_EINVAL, "timing stride %d < 1", every);
    std::lock_guard<std::mutex> lk(c->mu);
    c->tstride = every;
    return timing_reset(c);  // clears, keeps the selection
}

int bk_timing_select(bk_ctx *c, uint32_t mask) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->timing = mask;
    return timing_reset(c);
}

int bk_timing_read(bk_ctx *c, int kid, double *total_ms, int64_t *count) {
    if (!c || kid < 0 || kid >= BK_NUM_KERNELS) return fail(BK_EINVAL, "bad timing_read arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (!c->pending.empty()) {
        HIPCHK(hipStreamSynchronize(c->stream));
        for (auto &ev : c->pending) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
            c->tot_ms[ev.kid] += ms;
            c->cnt[ev.kid] += 1;
            c->pool.push_back(ev.a);
            c->pool.push_back(ev.b);
        }
        c->pending.clear();
    }
    if (total_ms) *total_ms = c->tot_ms[kid];
    if (count) *count = c->cnt[kid];
    return BK_OK;
}

}  // extern "C"
