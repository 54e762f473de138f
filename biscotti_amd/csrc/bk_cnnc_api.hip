// bk_cnnc_api.hip -- the one-layer cifar CNN's entries (include/bk.h
// bk_cnnc_shape): the evaluation set of the fifth kind and the
// CNNC RONI on two drawn mini-batches.  bk_eval / bk_block_finish_eval reach
// the kernel through eval_queue (bk_eval.hip); the kernel is k_cnnc (bk_cnnc.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "bk_ctx.h"

namespace bk {

int cnnc_check_shape(const bk_cnnc_shape *sh, CnncDims *out) {
    if (!sh) return fail(BK_EINVAL, "null shape");
    bool lds_ok = false;
    if (!cnnc_dims(sh->c_in, sh->h, sh->w, sh->k, sh->pad, sh->c_out, sh->n_classes, out, &lds_ok))
        return fail(BK_ENOTSUP,
                    "CNNC shape {c_in=%d, h=%d, w=%d, k=%d, pad=%d, c_out=%d, n_classes=%d} outside "
                    "1 <= c_in <= 4, 1 <= h, w <= 64, 1 <= k <= 5, 0 <= pad <= k, k <= h + 2 pad, "
                    "k <= w + 2 pad, 1 <= c_out <= 32, 2 <= n_classes <= 16",
                    (int)sh->c_in, (int)sh->h, (int)sh->w, (int)sh->k, (int)sh->pad, (int)sh->c_out,
                    (int)sh->n_classes);
    // right behind the limits: the band ring of 16 samples against a compute unit's LDS
    if (!lds_ok)
        return fail(BK_ENOTSUP, "CNNC shape needs %d bytes of LDS for its band ring (%d rows of %d planes), "
                    "more than 136 KiB", out->lds, out->D, out->c_in);
    return BK_OK;
}

// what both sets check after the shape, in the one-layer sets' order
static int check_samples(const CnncDims &m, const float *X, int64_t nv, int64_t ldv, const int32_t *y) {
    const int64_t din = (int64_t)m.c_in * m.h * m.w;
    if (nv < 1) return fail(BK_EINVAL, "need nv >= 1 (nv=%lld)", (long long)nv);
    if (ldv < din) return fail(BK_EINVAL, "ldv=%lld < c_in * h * w = %lld", (long long)ldv, (long long)din);
    if (nv > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "nv=%lld too large", (long long)nv);
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    for (int64_t i = 0; i < nv; ++i)
        if (y[i] < 0 || y[i] >= m.C)
            return fail(BK_EINVAL, "label y[%lld]=%d outside [0, %d)", (long long)i, (int)y[i], m.C);
    return BK_OK;
}

static int upload_samples(bk_ctx *c, const CnncDims &m, DevBuf &dX, DevBuf &dy, const float *X,
                          int64_t nv, int64_t ldv, const int32_t *y) {
    const size_t row = (size_t)m.c_in * m.h * m.w * sizeof(float);
    CHK(ensure(dX, (size_t)nv * row));
    CHK(ensure(dy, (size_t)nv * sizeof(int32_t)));
    HIPCHK(hipMemcpy2DAsync(dX.p, row, X, (size_t)ldv * sizeof(float), row, (size_t)nv,
                            hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dy.p, y, (size_t)nv * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BK_OK;
}

}  // namespace bk

int bk_eval_set_cnnc(bk_ctx *c, int set, const float *X, int64_t nv, int64_t ldv, const int32_t *y,
                     const bk_cnnc_shape *shape) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_index(set));
    CnncDims m;
    CHK(cnnc_check_shape(shape, &m));
    CHK(check_samples(m, X, nv, ldv, y));
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(eval_state(c));
    EvalSlot &s = c->eval->set[set];
    s.kind = EVAL_EMPTY;  // empty until the new set has landed
    HostDrain drain{c};
    CHK(upload_samples(c, m, s.X, s.y, X, nv, ldv, y));
    drain.armed = false;
    s.nv = nv;
    s.din = (int64_t)m.c_in * m.h * m.w;
    s.C = m.C;
    s.d = m.d;
    s.cnnc = m;
    s.kind = EVAL_CNNC;
    return BK_OK;
}

int bk_roni_cnnc_set_validation(bk_ctx *c, const float *Xv, int64_t nv, int64_t ldv, const int32_t *yv,
                                const bk_cnnc_shape *shape) {
    if (!c) return fail(BK_EINVAL, "null context");
    CnncDims m;
    CHK(cnnc_check_shape(shape, &m));
    CHK(check_samples(m, Xv, nv, ldv, yv));
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    c->cc_nv = 0;  // invalid until the new set has landed
    HostDrain drain{c};
    CHK(upload_samples(c, m, c->cc_X, c->cc_y, Xv, nv, ldv, yv));
    drain.armed = false;
    c->cc_dims = m;
    c->cc_nv = nv;
    return BK_OK;
}

// ww / deltas and the batches' indices to the device, k_cnnc on the 2 n
// evaluations, scores and near-tie counts back; synchronous
int bk_roni_cnnc_batches(bk_ctx *c, const double *ww, const double *deltas, int64_t n, int64_t ld,
                         const int64_t *idx, int64_t nb, double *scores, int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!idx && n > 0) return fail(BK_EINVAL, "null batch indices");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->cc_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_cnnc_set_validation");
    const CnncDims &m = c->cc_dims;
    const int64_t nv = c->cc_nv, d = m.d;
    if (n < 0) return fail(BK_EINVAL, "n=%lld < 0", (long long)n);
    if (n > 0 && ld < d) return fail(BK_EINVAL, "ld=%lld < the shape's d = %lld", (long long)ld, (long long)d);
    if (n > 262139) return fail(BK_ENOTSUP, "RONI n=%lld exceeds 262139", (long long)n);
    if (!ww || (n > 0 && (!deltas || !scores))) return fail(BK_EINVAL, "null pointer argument");
    if (idx && nb < 1) return fail(BK_EINVAL, "need a batch of nb >= 1 samples (nb=%lld)", (long long)nb);
    if (n == 0) return BK_OK;
    if (nb > ((int64_t)1 << 31) || 2 * n * (int64_t)cnnc_tiles(nb) > 0x7fffffff)
        return fail(BK_ENOTSUP, "the batches' %lld tiles exceed the grid", (long long)(2 * n * cnnc_tiles(nb)));
    const int64_t tiles = 2 * n * cnnc_tiles(nb);
    for (int64_t i = 0; i < 2 * n * nb; ++i)
        if (idx[i] < 0 || idx[i] >= nv)
            return fail(BK_EINVAL, "batch index %lld = %lld outside [0, %lld)", (long long)i,
                        (long long)idx[i], (long long)nv);
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: queued H2D copies may still read ww / deltas
    const size_t words = (size_t)4 * n + 1;
    CHK(ensure(c->roni_w, (size_t)d * sizeof(double)));
    CHK(ensure(c->roni_d, (size_t)n * d * sizeof(double)));
    CHK(ensure(c->roni_s, (size_t)n * sizeof(double)));
    CHK(ensure(c->rmc_nt, (size_t)2 * n * sizeof(int32_t)));
    CHK(ensure(c->rmc_idx, (size_t)2 * n * nb * sizeof(int64_t)));
    const size_t had = c->cnn_cnt.bytes;
    CHK(ensure(c->cnn_cnt, words * sizeof(unsigned int)));
    if (c->cnn_cnt.bytes != had)  // grown: zero once, every launch leaves it zero
        HIPCHK(hipMemsetAsync(c->cnn_cnt.p, 0, c->cnn_cnt.bytes, c->stream));
    double *dw = (double *)c->roni_w.p, *dd = (double *)c->roni_d.p, *ds = (double *)c->roni_s.p;
    int32_t *dnt = (int32_t *)c->rmc_nt.p;
    HIPCHK(hipMemcpyAsync(dw, ww, (size_t)d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpy2DAsync(dd, (size_t)d * sizeof(double), deltas, (size_t)ld * sizeof(double),
                            (size_t)d * sizeof(double), (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->rmc_idx.p, idx, (size_t)2 * n * nb * sizeof(int64_t), hipMemcpyHostToDevice,
                          c->stream));
    CnncLaunch a = {};
    a.desc.nsets = 1;
    a.desc.s[0] = {c->cc_X.p, c->cc_y.p, nullptr, nv, (int64_t)m.c_in * m.h * m.w, 0};
    a.m = m;
    a.ww = dw;
    a.deltas = dd;
    a.ld = d;
    a.idx = (const int64_t *)c->rmc_idx.p;
    a.nb = nb;
    a.n = n;
    a.cnt = (unsigned int *)c->cnn_cnt.p;
    a.scores = ds;
    a.near = dnt;
    const hipError_t he = launch_cnnc(a, tiles, c->stream);
    if (he != hipSuccess) return fail(BK_EHIP, "k_cnnc launch: %s", hipGetErrorString(he));
    HIPCHK(hipMemcpyAsync(scores, ds, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (near_ties)
        HIPCHK(hipMemcpyAsync(near_ties, dnt, (size_t)2 * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                              c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    return BK_OK;
}
