// bk_batch.hip -- bk_multikrum_batch*: `batch` independent Multi-Krum problems
// of one shape (n, d, f) in one call (include/bk.h).  Within k_small's range
// (small_ok: n <= 128, d <= 32,768, the small path on) the problems run as
// k_small_batch / k_tiny_batch launches (bk_small_batch.hip) of W problems each, W
// bounded by the partials' workspace budget; every other shape, and batch = 1,
// runs the single-problem device path once per problem on the context stream.
// Either way problem b's outputs and record are bitwise bk_multikrum_device's
// on that problem alone.  bk_multikrum_ragged* (below them) is the same call
// with a row count and an f per problem: the problems go by ceil(n / 16) into
// groups that share k_small_ragged / k_tiny_ragged launches
// (bk_small_ragged.hip), everything else runs the single path in the same call.
#include <string.h>

#include <algorithm>

#include "bk_ctx.h"

namespace bk {

// the next slot of the pinned ring, `bytes` large, free to write: the call
// that used it last has had its copy run (its event).  Shared with the RONI
// rounds' batch indices (bk_entries.hip)
int ragged_stage_slot(bk_ctx *c, size_t bytes, int *slot) {
    const int s = c->ragged_next;
    c->ragged_next = (s + 1) % bk_ctx::RAGGED_SLOTS;
    if (!c->ev_ragged[s])
        HIPCHK(hipEventCreateWithFlags(&c->ev_ragged[s], hipEventDisableTiming));
    if (c->ragged_used[s]) HIPCHK(hipEventSynchronize(c->ev_ragged[s]));
    c->ragged_used[s] = false;
    if (c->ragged_stage_bytes[s] < bytes) {
        if (c->ragged_stage[s]) (void)hipHostFree(c->ragged_stage[s]);
        c->ragged_stage[s] = nullptr;
        c->ragged_stage_bytes[s] = 0;
        const size_t want = bytes < 4096 ? 4096 : bytes;
        const hipError_t e = hipHostMalloc(&c->ragged_stage[s], want, hipHostMallocPortable);
        if (e != hipSuccess) {
            c->ragged_stage[s] = nullptr;
            return fail(BK_ENOMEM, "hipHostMalloc(%zu bytes): %s", want, hipGetErrorString(e));
        }
        c->ragged_stage_bytes[s] = want;
    }
    *slot = s;
    return BK_OK;
}

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
// one problem of a batch by the single device path, its record copied to place
// b of the batch record store (batch_rec holds that many)
int run_one_of_batch(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                     int64_t f, int64_t *d_sel, double *d_scores, double *d_mean, int64_t b) {
    auto run = [&] { return run_device(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean); };
    if (certified(c, dtype))
        CHK(run_certified(c, run));
    else
        CHK(run());
    // the finish wrote the context's mapped record (written back at its
    // kernel's end): stream order puts this copy behind it
    HIPCHK(hipMemcpyAsync((double *)c->batch_rec.p + b * MARGIN_WORDS, c->hmargin,
                          MARGIN_WORDS * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return BK_OK;
}

int run_batch_loop(bk_ctx *c, const void *dX, int dtype, int64_t batch, int64_t n, int64_t d,
                   int64_t ld, int64_t stride, int64_t f, int64_t *d_sel, double *d_scores,
                   double *d_mean) {
    CHK(ensure(c->batch_rec, (size_t)batch * MARGIN_WORDS * sizeof(double)));
    const int64_t m = n - f;
    const size_t es = esize(dtype);
    for (int64_t b = 0; b < batch; ++b)
        CHK(run_one_of_batch(c, (const char *)dX + (size_t)b * stride * es, dtype, n, d, ld, f,
                             d_sel + b * m, d_scores ? d_scores + b * n : nullptr,
                             d_mean ? d_mean + b * d : nullptr, b));
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

// ---- bk_multikrum_ragged*: every problem with its own n and f ----------------

// the checks of both entries, in the header's order; all of them come before
// the first use of the context (sel_name: the entry's name for its sel argument)
int check_ragged(bk_ctx *c, const void *X, int dtype, int64_t batch, const int64_t *offsets,
                 const int64_t *fs, int64_t d, int64_t ld, const void *sel, const char *sel_name) {
    if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype %d", dtype);
    if (batch < 1) return fail(BK_EINVAL, "need batch >= 1 (batch=%lld)", (long long)batch);
    if (batch > BK_MAX_BATCH)
        return fail(BK_ENOTSUP, "batch=%lld exceeds BK_MAX_BATCH=%d", (long long)batch, BK_MAX_BATCH);
    if (d < 1) return fail(BK_EINVAL, "need d >= 1 (d=%lld)", (long long)d);
    if (ld < d) return fail(BK_EINVAL, "ld=%lld < d=%lld", (long long)ld, (long long)d);
    if (!c) return fail(BK_EINVAL, "null context");
    if (!X) return fail(BK_EINVAL, "null X");
    if (!offsets) return fail(BK_EINVAL, "null offsets");
    if (!fs) return fail(BK_EINVAL, "null fs");
    if (!sel) return fail(BK_EINVAL, "null %s", sel_name);
    if (offsets[0] != 0)
        return fail(BK_EINVAL, "offsets[0] = %lld, not 0", (long long)offsets[0]);
    for (int64_t b = 0; b < batch; ++b)
        if (offsets[b + 1] <= offsets[b])
            return fail(BK_EINVAL, "problem %lld: n = offsets[%lld] - offsets[%lld] = %lld, need n >= 1",
                        (long long)b, (long long)b + 1, (long long)b,
                        (long long)((uint64_t)offsets[b + 1] - (uint64_t)offsets[b]));
    for (int64_t b = 0; b < batch; ++b) {
        const int st = bk_check_args(offsets[b + 1] - offsets[b], d, fs[b]);
        if (st != BK_OK) {
            const std::string why = g_err;
            return fail(st, "problem %lld: %s", (long long)b, why.c_str());
        }
    }
    return BK_OK;
}

constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// bk_multikrum_ragged_device past its checks.  The problems within k_small's
// range go by NB = ceil(n_b / 16) into buckets: small_plan depends on n only
// through NB and on d through P and C, so inside a bucket the partials' stride,
// the G and M item counts and the kernel instantiation the single call picks
// are one -- only the same instantiation gives the single call's bits.  Each
// bucket of two or more runs as k_small_ragged<T, VEC, NB> launches of W
// problems (bk_small_ragged.hip), W bounded as run_small_batch's; the NB = 1
// bucket within k_tiny's range as ONE k_tiny_ragged launch.  The descriptors
// and the launches' segment starts go up in one copy through the pinned ring;
// the kernels write every output at the caller's position.  Every other
// problem, a bucket's only one and batch = 1 run the single device path on the
// same stream, the record copied behind each (run_one_of_batch).
int run_ragged_device(bk_ctx *c, const void *dX, int dtype, int64_t batch, const int64_t *offsets,
                      const int64_t *fs, int64_t d, int64_t ld, int64_t *d_sel, double *d_scores,
                      double *d_mean) {
    c->batch_one = 0;
    if (batch == 1) {
        // the single call itself, at its own cost (run_batch_device)
        auto run = [&] {
            return run_device(c, dX, dtype, offsets[1], d, ld, fs[0], d_sel, d_scores, d_mean);
        };
        if (certified(c, dtype))
            CHK(run_certified(c, run));
        else
            CHK(run());
        c->batch_one = 1;
        c->batch_last = 1;
        return BK_OK;
    }
    const size_t ub = (size_t)batch, es = esize(dtype);
    std::vector<int64_t> selo(ub + 1, 0);  // problem b's sel at sum_{c<b} m_c
    std::vector<int64_t> bucket[9], single;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        selo[(size_t)b + 1] = selo[(size_t)b] + n - fs[b];
        if (small_ok(c, dX, dtype, n, d, ld))
            bucket[(n + 15) / 16].push_back(b);
        else
            single.push_back(b);
    }
    struct Launch {
        int NB, W;
        size_t first, seg;  // its first descriptor; its segment starts (in int32s)
        bool tiny;
        SmallPlan sp;
        size_t pstride;
    };
    std::vector<Launch> launches;
    std::vector<int64_t> kern;  // the kernels' problems, in launch order
    size_t nseg = 0, part_bytes = 0;
    int maxW = 0;
    const size_t ws = batch_ws_bytes();
    for (int NB = 1; NB <= 8; ++NB) {
        const std::vector<int64_t> &bk = bucket[NB];
        if (bk.size() == 1) single.push_back(bk[0]);
        if (bk.size() < 2) continue;
        const SmallPlan sp = small_plan(16 * NB, d, c->num_cu);
        if (NB == 1 && tiny_ok(16, d)) {  // one workgroup per problem, no queue
            launches.push_back({NB, (int)bk.size(), kern.size(), 0, true, sp, 0});
            kern.insert(kern.end(), bk.begin(), bk.end());
            continue;
        }
        // per problem and chunk: the full-square partial Gram (16 NB)^2 + its diagonal (run_small)
        const size_t np16 = (size_t)16 * NB;
        const size_t pstride = (size_t)sp.P * (np16 * np16 + np16);
        const int64_t fit = (int64_t)(ws / (pstride * sizeof(double)));
        const size_t maxw = (size_t)std::min<int64_t>(std::max<int64_t>(fit, 1), SMALL_BATCH_MAX_W);
        for (size_t b0 = 0; b0 < bk.size(); b0 += maxw) {
            const int w = (int)std::min(maxw, bk.size() - b0);
            launches.push_back({NB, w, kern.size(), nseg, false, sp, pstride});
            nseg += (size_t)w + 2;
            maxW = std::max(maxW, w);
            part_bytes = std::max(part_bytes, (size_t)w * pstride * sizeof(double));
            kern.insert(kern.end(), bk.begin() + b0, bk.begin() + b0 + w);
        }
    }
    CHK(ensure(c->batch_rec, ub * MARGIN_WORDS * sizeof(double)));
    if (!launches.empty()) {
        if (maxW > 0) {
            CHK(ensure(c->batch_part, part_bytes));
            const size_t lbytes = (size_t)(1 + maxW) * SMALL_CTR_WORDS * sizeof(unsigned);
            if (c->batch_ctr.bytes < lbytes) {  // zeroed once; every launch leaves them zero
                CHK(ensure(c->batch_ctr, lbytes));
                HIPCHK(hipMemsetAsync(c->batch_ctr.p, 0, c->batch_ctr.bytes, c->stream));
            }
        }
        const size_t rows = (size_t)offsets[batch];
        CHK(ensure(c->batch_diag, rows * sizeof(double)));
        double *sc = d_scores;
        if (!sc) {
            CHK(ensure(c->batch_scores, rows * sizeof(double)));
            sc = (double *)c->batch_scores.p;
        }
        // the staging block: descriptors | segment starts
        const size_t off_seg = up16(kern.size() * sizeof(RaggedBatchDesc));
        const size_t sbytes = off_seg + nseg * sizeof(int32_t);
        CHK(ensure(c->batch_desc, sbytes));
        int slot = 0;
        CHK(ragged_stage_slot(c, sbytes, &slot));
        char *hs = (char *)c->ragged_stage[slot];
        RaggedBatchDesc *hd = (RaggedBatchDesc *)hs;
        int32_t *hseg = (int32_t *)(hs + off_seg);
        for (const Launch &L : launches) {
            int32_t nn[SMALL_BATCH_MAX_W];
            for (int q = 0; q < L.W; ++q) {
                const int64_t b = kern[L.first + q], n = offsets[b + 1] - offsets[b];
                RaggedBatchDesc &r = hd[L.first + q];
                r.n = (int32_t)n;
                r.f = (int32_t)fs[b];
                r.m = (int32_t)(n - fs[b]);
                r.idx = (int32_t)b;
                r.row = offsets[b];
                r.sc = offsets[b];
                r.so = selo[(size_t)b];
                r.slot = q;
                r.pad = 0;
                if (!L.tiny) nn[q] = (int32_t)n;
            }
            if (!L.tiny)
                ragged_batch_seg_build(nn, L.W, SMALL_SPLIT_ITEMS * L.sp.P, d_mean ? L.sp.C : 1,
                                       hseg + L.seg);
        }
        CHK(timed(c, BK_K_H2D, [&] {
            return hipMemcpyAsync(c->batch_desc.p, hs, sbytes, hipMemcpyHostToDevice, c->stream);
        }));
        HIPCHK(hipEventRecord(c->ev_ragged[slot], c->stream));
        c->ragged_used[slot] = true;
        const char *ds = (const char *)c->batch_desc.p;
        for (const Launch &L : launches) {
            const RaggedBatchDesc *dd = (const RaggedBatchDesc *)ds + L.first;
            if (L.tiny) {
                CHK(timed(c, BK_K_SMALL, [&] {
                    return launch_tiny_ragged(dX, dtype, ld, L.W, d, dd, sc, (double *)c->batch_diag.p,
                                              d_sel, d_mean, (double *)c->batch_rec.p, c->stream);
                }));
                continue;
            }
            const uint64_t spin = next_spin(c);
            CHK(timed(c, BK_K_SMALL, [&] {
                return launch_small_ragged(dX, dtype, ld, L.W, L.NB, d, L.sp, dd,
                                           (const int32_t *)(ds + off_seg) + L.seg,
                                           hseg[L.seg + L.W + 1], (double *)c->batch_part.p,
                                           (int64_t)L.pstride, sc, (double *)c->batch_diag.p, d_sel,
                                           d_mean, (double *)c->batch_rec.p,
                                           (unsigned *)c->batch_ctr.p, c->num_cu, c->stream, spin);
            }));
        }
    }
    for (const int64_t b : single)
        CHK(run_one_of_batch(c, (const char *)dX + (size_t)offsets[b] * (size_t)ld * es, dtype,
                             offsets[b + 1] - offsets[b], d, ld, fs[b], d_sel + selo[(size_t)b],
                             d_scores ? d_scores + offsets[b] : nullptr,
                             d_mean ? d_mean + b * d : nullptr, b));
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

int bk_multikrum_ragged_device(bk_ctx *c, const void *dX, int dtype, int64_t batch,
                               const int64_t *offsets, const int64_t *fs, int64_t d, int64_t ld,
                               int64_t *d_sel, double *d_scores, double *d_mean) {
    CHK(check_ragged(c, dX, dtype, batch, offsets, fs, d, ld, d_sel, "d_sel_idx"));
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return run_ragged_device(c, dX, dtype, batch, offsets, fs, d, ld, d_sel, d_scores, d_mean);
}

int bk_multikrum_ragged(bk_ctx *c, const void *X, int where, int dtype, int64_t batch,
                        const int64_t *offsets, const int64_t *fs, int64_t d, int64_t ld,
                        int64_t *sel_idx, int64_t *m_out, double *scores, double *mean_out) {
    CHK(check_ragged(c, X, dtype, batch, offsets, fs, d, ld, sel_idx, "sel_idx"));
    if (where != BK_HOST && where != BK_HOST_PINNED)
        return fail(BK_EINVAL, "bad where=%d (the ragged host entry takes host rows)", where);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    const size_t es = esize(dtype);
    const size_t rows = (size_t)offsets[batch];
    size_t nsel = 0;
    for (int64_t b = 0; b < batch; ++b) nsel += (size_t)(offsets[b + 1] - offsets[b] - fs[b]);
    const size_t span = (rows - 1) * (size_t)ld + (size_t)d;  // elements
    CHK(ensure(c->batch_X, span * es));
    CHK(ensure(c->batch_sel, nsel * sizeof(int64_t)));
    if (scores) CHK(ensure(c->batch_hsc, rows * sizeof(double)));
    if (mean_out) CHK(ensure(c->batch_mean, (size_t)batch * d * sizeof(double)));
    HostDrain hd{c};
    // one copy of the whole packed matrix (the kernels never read host memory)
    CHK(timed(c, BK_K_H2D, [&] {
        return hipMemcpyAsync(c->batch_X.p, X, span * es, hipMemcpyHostToDevice, c->stream);
    }));
    int64_t *dsel = (int64_t *)c->batch_sel.p;
    double *dsc = scores ? (double *)c->batch_hsc.p : nullptr;
    double *dmean = mean_out ? (double *)c->batch_mean.p : nullptr;
    CHK(run_ragged_device(c, c->batch_X.p, dtype, batch, offsets, fs, d, ld, dsel, dsc, dmean));
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(sel_idx, dsel, nsel * sizeof(int64_t), hipMemcpyDeviceToHost,
                                      c->stream);
        if (e == hipSuccess && scores)
            e = hipMemcpyAsync(scores, dsc, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && mean_out)
            e = hipMemcpyAsync(mean_out, dmean, (size_t)batch * d * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream);
        return e;
    }));
    HIPCHK(wait_stream(c));
    hd.armed = false;
    if (m_out)
        for (int64_t b = 0; b < batch; ++b) m_out[b] = offsets[b + 1] - offsets[b] - fs[b];
    double mg[MARGIN_WORDS];
    return read_margin(c, mg);  // the stream is done: the records' error codes
}

int bk_ragged_batch_queue_item(const int32_t *n, int W, int NGI, int C, int64_t item, int *p,
                               int *it) {
    if (!n || !p || !it) return fail(BK_EINVAL, "null n / p / it");
    if (W < 1 || W > SMALL_BATCH_MAX_W || NGI < 1 || C < 1)
        return fail(BK_EINVAL, "need 1 <= W <= %d, NGI >= 1 and C >= 1 (W=%d NGI=%d C=%d)",
                    SMALL_BATCH_MAX_W, W, NGI, C);
    for (int j = 0; j < W; ++j)
        if (n[j] < 1 || n[j] > 128) return fail(BK_EINVAL, "n[%d] = %d outside 1..128", j, (int)n[j]);
    if (NGI > 1024 || C > 512)
        return fail(BK_EINVAL, "NGI=%d / C=%d past k_small's range (1,024 / 512)", NGI, C);
    std::vector<int32_t> seg((size_t)W + 2);
    ragged_batch_seg_build(n, W, NGI, C, seg.data());
    if (item < 0 || item >= seg[(size_t)W + 1])
        return fail(BK_EINVAL, "item %lld outside the queue (0..%d)", (long long)item,
                    (int)seg[(size_t)W + 1] - 1);
    ragged_batch_queue_decode(seg.data(), W, NGI, (int)item, *p, *it);
    return BK_OK;
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
