// bk_batch.hip -- bk_multikrum_batch*: `batch` independent Multi-Krum problems
// of one shape (n, d, f) in one call (include/bk.h).  Within k_small's range
// (small_ok: n <= 128, d <= 32,768, the small path on) the problems run as
// k_small_batch / k_tiny_batch launches (bk_small_batch.hip) of W problems each, W
// bounded by the partials' workspace budget; every other shape, and batch = 1,
// runs the single-problem device path once per problem on the context stream.
// Either way problem b's outputs and record are bitwise bk_multikrum_device's
// on that problem alone.
#include <string.h>

#include <algorithm>

#include "bk_ctx.h"

namespace bk {

namespace {

// the partials of one launch: BK_BATCH_WS_BYTES, read at the call; it may only
// lower the default (1 GiB)
size_t batch_ws_bytes() {
    const size_t dflt = (size_t)1 << 30;
    const char *e = getenv("BK_BATCH_WS_BYTES");
    if (!e) return dflt;
    const long long v = atoll(e);
    return v > 0 && (size_t)v < dflt ? (size_t)v : dflt;
}

// shape checks first: they need no context, so they work with no GPU present
int check_batch(bk_ctx *c, const void *X, int dtype, int64_t batch, int64_t n, int64_t d,
                int64_t ld, int64_t stride, int64_t f) {
    if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype %d", dtype);
    if (batch < 1) return fail(BK_EINVAL, "need batch >= 1 (batch=%lld)", (long long)batch);
    if (batch > BK_MAX_BATCH)
        return fail(BK_ENOTSUP, "batch=%lld exceeds BK_MAX_BATCH=%d", (long long)batch, BK_MAX_BATCH);
    CHK(bk_check_args(n, d, f));
    if (ld < d) return fail(BK_EINVAL, "ld=%lld < d=%lld", (long long)ld, (long long)d);
    if (stride < (n - 1) * ld + d)
        return fail(BK_EINVAL, "stride=%lld < (n-1)*ld + d = %lld: the problems overlap",
                    (long long)stride, (long long)((n - 1) * ld + d));
    if (!c) return fail(BK_EINVAL, "null context");
    if (!X) return fail(BK_EINVAL, "null X");
    return BK_OK;
}

// the whole batch as k_small_batch / k_tiny_batch launches of W problems
int run_small_batch(bk_ctx *c, const void *dX, int dtype, int64_t batch, int64_t n, int64_t d,
                    int64_t ld, int64_t stride, int64_t f, int64_t *d_sel, double *d_scores,
                    double *d_mean) {
    const SmallPlan sp = small_plan((int)n, d, c->num_cu);
    const bool tiny = tiny_ok((int)n, d);
    // per problem and chunk: the full-square partial Gram (16 nb16)^2 + its diagonal (run_small)
    const size_t np16 = (size_t)16 * sp.nb16;
    const size_t pstride = (size_t)sp.P * (np16 * np16 + np16);
    int64_t W = batch;
    if (!tiny) {
        const int64_t fit = (int64_t)(batch_ws_bytes() / (pstride * sizeof(double)));
        W = std::min<int64_t>(W, std::max<int64_t>(fit, 1));
        W = std::min<int64_t>(W, SMALL_BATCH_MAX_W);
        CHK(ensure(c->batch_part, (size_t)W * pstride * sizeof(double)));
        const size_t lbytes = (size_t)(1 + W) * SMALL_CTR_WORDS * sizeof(unsigned);
        if (c->batch_ctr.bytes < lbytes) {  // zeroed once; every launch leaves them zero
            CHK(ensure(c->batch_ctr, lbytes));
            HIPCHK(hipMemsetAsync(c->batch_ctr.p, 0, c->batch_ctr.bytes, c->stream));
        }
    }
    CHK(ensure(c->batch_diag, (size_t)batch * n * sizeof(double)));
    CHK(ensure(c->batch_rec, (size_t)batch * MARGIN_WORDS * sizeof(double)));
    double *sc = d_scores;
    if (!sc) {
        CHK(ensure(c->batch_scores, (size_t)batch * n * sizeof(double)));
        sc = (double *)c->batch_scores.p;
    }
    const int64_t m = n - f;
    const size_t es = esize(dtype);
    for (int64_t b0 = 0; b0 < batch; b0 += W) {
        const int w = (int)std::min<int64_t>(W, batch - b0);
        const uint64_t spin = next_spin(c);
        CHK(timed(c, BK_K_SMALL, [&] {
            return launch_small_batch((const char *)dX + (size_t)b0 * stride * es, dtype, ld, stride,
                                      w, (int)n, d, (int)f, sp, (double *)c->batch_part.p,
                                      (int64_t)pstride, sc + b0 * n,
                                      (double *)c->batch_diag.p + b0 * n, d_sel + b0 * m,
                                      d_mean ? d_mean + b0 * d : nullptr,
                                      (double *)c->batch_rec.p + b0 * MARGIN_WORDS,
                                      (unsigned *)c->batch_ctr.p, c->num_cu, c->stream, spin);
        }));
    }
    return BK_OK;
}

// the single-problem device path once per problem (the f32 / f64 modes and
// certification apply per problem), each problem's record copied behind it
int run_batch_loop(bk_ctx *c, const void *dX, int dtype, int64_t batch, int64_t n, int64_t d,
                   int64_t ld, int64_t stride, int64_t f, int64_t *d_sel, double *d_scores,
                   double *d_mean) {
    CHK(ensure(c->batch_rec, (size_t)batch * MARGIN_WORDS * sizeof(double)));
    const int64_t m = n - f;
    const size_t es = esize(dtype);
    for (int64_t b = 0; b < batch; ++b) {
        auto run = [&] {
            return run_device(c, (const char *)dX + (size_t)b * stride * es, dtype, n, d, ld, f,
                              d_sel + b * m, d_scores ? d_scores + b * n : nullptr,
                              d_mean ? d_mean + b * d : nullptr);
        };
        if (certified(c, dtype))
            CHK(run_certified(c, run));
        else
            CHK(run());
        // the finish wrote the context's mapped record (written back at its
        // kernel's end): stream order puts this copy behind it
        HIPCHK(hipMemcpyAsync((double *)c->batch_rec.p + b * MARGIN_WORDS, c->hmargin,
                              MARGIN_WORDS * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return BK_OK;
}

int run_batch_device(bk_ctx *c, const void *dX, int dtype, int64_t batch, int64_t n, int64_t d,
                     int64_t ld, int64_t stride, int64_t f, int64_t *d_sel, double *d_scores,
                     double *d_mean) {
    c->batch_one = 0;
    if (batch == 1) {
        // the single call itself, at its own cost: its record stays where that
        // call leaves it (the context's mapped record)
        auto run = [&] { return run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean); };
        if (certified(c, dtype))
            CHK(run_certified(c, run));
        else
            CHK(run());
        c->batch_one = 1;
        c->batch_last = 1;
        return BK_OK;
    }
    if (small_ok(c, dX, dtype, n, d, ld))
        CHK(run_small_batch(c, dX, dtype, batch, n, d, ld, stride, f, d_sel, d_scores, d_mean));
    else
        CHK(run_batch_loop(c, dX, dtype, batch, n, d, ld, stride, f, d_sel, d_scores, d_mean));
    c->margin_valid = 1;
    c->margin_host = c->batch_pick;
    c->margin_unchecked = 1;
    c->batch_last = batch;
    c->batch_fetched = 0;
    return BK_OK;
}

}  // namespace

// The records of the last batched call, once its stream is done: all of them
// into batch_rec_h, and into batch_pick the one bk_selection_margin* reports --
// a record with an error code if there is one (a give-up marks them all), else
// the lowest-index problem's with near_tie = 1, else the one with the smallest
// gap - err_bound
int batch_fetch(bk_ctx *c) {
    if (c->batch_fetched) return BK_OK;
    const int64_t B = c->batch_last;
    c->batch_rec_h.resize((size_t)B * MARGIN_WORDS);
    HIPCHK(hipMemcpyAsync(c->batch_rec_h.data(), c->batch_rec.p,
                          (size_t)B * MARGIN_WORDS * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    batch_pick_record(c);
    return BK_OK;
}

// batch_pick from the batch_last records in batch_rec_h (a synchronous caller
// that has them on the host already -- bk_collect_finish_batch -- calls this
// itself and no fetch follows)
void batch_pick_record(bk_ctx *c) {
    const int64_t B = c->batch_last;
    const double *r = c->batch_rec_h.data();
    int64_t pick = -1;
    for (int64_t b = 0; b < B && pick < 0; ++b)
        if (r[b * MARGIN_WORDS + 2] >= 2.0) pick = b;  // MARGIN_* error codes
    for (int64_t b = 0; b < B && pick < 0; ++b)
        if (r[b * MARGIN_WORDS + 2] != 0.0) pick = b;
    if (pick < 0) {
        pick = 0;
        for (int64_t b = 1; b < B; ++b)
            if (r[b * MARGIN_WORDS] - r[b * MARGIN_WORDS + 1] <
                r[pick * MARGIN_WORDS] - r[pick * MARGIN_WORDS + 1])
                pick = b;
    }
    memcpy(c->batch_pick, r + pick * MARGIN_WORDS, sizeof c->batch_pick);
    c->batch_fetched = 1;
}

}  // namespace bk

extern "C" {

int bk_multikrum_batch_device(bk_ctx *c, const void *dX, int dtype, int64_t batch, int64_t n,
                              int64_t d, int64_t ld, int64_t stride, int64_t f, int64_t *d_sel,
                              double *d_scores, double *d_mean) {
    CHK(check_batch(c, dX, dtype, batch, n, d, ld, stride, f));
    if (!d_sel) return fail(BK_EINVAL, "null d_sel_idx");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return run_batch_device(c, dX, dtype, batch, n, d, ld, stride, f, d_sel, d_scores, d_mean);
}

int bk_multikrum_batch(bk_ctx *c, const void *X, int where, int dtype, int64_t batch, int64_t n,
                       int64_t d, int64_t ld, int64_t stride, int64_t f, int64_t *sel_idx,
                       int64_t *m_out, double *scores, double *mean_out) {
    CHK(check_batch(c, X, dtype, batch, n, d, ld, stride, f));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    if (where != BK_HOST && where != BK_HOST_PINNED)
        return fail(BK_EINVAL, "bad where=%d (the batched host entry takes host rows)", where);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    const size_t es = esize(dtype);
    const int64_t m = n - f;
    const size_t span = (size_t)(batch - 1) * stride + (size_t)(n - 1) * ld + d;  // elements
    CHK(ensure(c->batch_X, span * es));
    CHK(ensure(c->batch_sel, (size_t)batch * m * sizeof(int64_t)));
    if (scores) CHK(ensure(c->batch_hsc, (size_t)batch * n * sizeof(double)));
    if (mean_out) CHK(ensure(c->batch_mean, (size_t)batch * d * sizeof(double)));
    HostDrain hd{c};
    // one copy of the whole batch (the kernels never read host memory)
    CHK(timed(c, BK_K_H2D, [&] {
        return hipMemcpyAsync(c->batch_X.p, X, span * es, hipMemcpyHostToDevice, c->stream);
    }));
    int64_t *dsel = (int64_t *)c->batch_sel.p;
    double *dsc = scores ? (double *)c->batch_hsc.p : nullptr;
    double *dmean = mean_out ? (double *)c->batch_mean.p : nullptr;
    CHK(run_batch_device(c, c->batch_X.p, dtype, batch, n, d, ld, stride, f, dsel, dsc, dmean));
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(sel_idx, dsel, (size_t)batch * m * sizeof(int64_t),
                                      hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && scores)
            e = hipMemcpyAsync(scores, dsc, (size_t)batch * n * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && mean_out)
            e = hipMemcpyAsync(mean_out, dmean, (size_t)batch * d * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream);
        return e;
    }));
    HIPCHK(wait_stream(c));
    hd.armed = false;
    if (m_out) *m_out = m;
    double mg[MARGIN_WORDS];
    return read_margin(c, mg);  // the stream is done: the records' error codes
}

int bk_selection_margin_batch(bk_ctx *c, double *records, int64_t batch) {
    if (!c || !records) return fail(BK_EINVAL, "null context / records");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    // (a batch of 1 is the single call: its record is the context's own)
    const bool one = c->batch_one && c->margin_host == c->hmargin;
    if (!c->margin_valid || !(one || c->margin_host == c->batch_pick))
        return fail(BK_EINVAL, "the last Multi-Krum call on this context was not a batched one");
    if (batch != c->batch_last)
        return fail(BK_EINVAL, "batch=%lld, but the last batched call had %lld problems",
                    (long long)batch, (long long)c->batch_last);
    double mg[MARGIN_WORDS];
    CHK(read_margin(c, mg));
    if (one) {
        memcpy(records, mg, 8 * sizeof(double));
        return BK_OK;
    }
    for (int64_t b = 0; b < batch; ++b)  // the public record (u_G stays internal)
        memcpy(records + 8 * b, c->batch_rec_h.data() + (size_t)b * MARGIN_WORDS, 8 * sizeof(double));
    return BK_OK;
}

}  // extern "C"
