// bk_grad_cnn2_api.hip -- the host side of bk_grad_set_cnn2 / bk_grad_cnn2
// (include/bk.h; the kernels: bk_grad_cnn2.hip; the state: bk_ctx.h struct
// GradCnn2 inside Grad).  The two-layer CNN peer's privateFun on
// its resident shard: four launches (forward, backward, sum, tail), synchronous.
// The argument handling is the softmax step's (bk_grad_api.hip).
#include <hip/hip_runtime.h>
#include <math.h>

#include <mutex>

#include "bk_ctx.h"

int bk_grad_set_cnn2(bk_ctx *c, const float *X, int64_t nn, int64_t ldx, const int32_t *y,
                     const bk_cnn2_shape *shape) {
    if (!c) return fail(BK_EINVAL, "null context");
    Cnn2Dims m;
    CHK(cnn2_check_shape(shape, &m));
    GradCnn2Plan p;
    if (!grad_cnn2_plan(m, &p))
        return fail(BK_ENOTSUP, "the CNN2 shape's gradient step is outside the 128 KiB of LDS of its kernels");
    const int64_t din = (int64_t)m.c_in * m.h * m.w;
    if (nn < 1) return fail(BK_EINVAL, "need nn >= 1 (nn=%lld)", (long long)nn);
    if (ldx < din) return fail(BK_EINVAL, "ldx=%lld < c_in * h * w = %lld", (long long)ldx, (long long)din);
    if (nn > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "nn=%lld too large", (long long)nn);
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    for (int64_t i = 0; i < nn; ++i)
        if (y[i] < 0 || y[i] >= m.C)
            return fail(BK_EINVAL, "label y[%lld]=%d outside [0, %d)", (long long)i, (int)y[i], m.C);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(grad_state(c));
    Grad *g = c->grad;
    g->kind = EVAL_EMPTY;  // empty until the new set has landed
    HostDrain drain{c};
    const size_t row = (size_t)din * sizeof(float);
    CHK(ensure(g->X, (size_t)nn * row));
    CHK(ensure(g->y, (size_t)nn * sizeof(int32_t)));
    HIPCHK(hipMemcpy2DAsync(g->X.p, row, X, (size_t)ldx * sizeof(float), row, (size_t)nn,
                            hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->y.p, y, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    g->nn = nn;
    g->din = din;
    g->C = m.C;
    g->d = m.d;
    g->cnn2.m = m;
    g->cnn2.p = p;
    g->kind = EVAL_CNN2;
    return BK_OK;
}

int bk_grad_cnn2(bk_ctx *c, const double *ww, int where, const int64_t *idx, int64_t count,
                 double max_norm, const double *noise, int precision, double *delta_out,
                 int64_t *q_out, double *loss_out, double *norm_out) {
    CHK(grad_check_call(c, ww, where, precision, delta_out, q_out));
    if (!isfinite(max_norm) || !(max_norm > 0.0))
        return fail(BK_EINVAL, "max_norm=%g is not a positive finite number", max_norm);
    std::lock_guard<std::mutex> lk(c->mu);
    int64_t n = 0;
    CHK(grad_check_batch(c, EVAL_CNN2, idx, count, GRAD_CNN2_MAX_BATCH, &n));
    Grad *g = c->grad;
    GradCnn2 &gc = g->cnn2;
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: the queued copies may still read the caller's memory
    GradIO io;
    CHK(grad_stage_call(c, g, ww, where, idx, n, noise, delta_out, q_out, &io));
    CHK(ensure(gc.scr, (size_t)n * (size_t)gc.p.stride));
    CHK(ensure(g->part, (size_t)g->d * 8));
    CHK(ensure(gc.ssq, (size_t)((g->d + 255) / 256) * 8));
    CHK(ensure(gc.scal, 64));
    GradCnn2Args a = {};
    a.X = (const float *)g->X.p;
    a.y = (const int32_t *)g->y.p;
    a.ww = io.ww;
    a.noise = io.noise;
    a.rows = io.rows;
    a.count = n;
    a.nn = g->nn;
    a.m = gc.m;
    a.p = gc.p;
    a.max_norm = max_norm;
    a.scale = grad_scale_of(precision);
    a.scr = (char *)gc.scr.p;
    a.G = (double *)g->part.p;
    a.ssq = (double *)gc.ssq.p;
    a.scal = (double *)gc.scal.p;
    a.delta = io.delta;
    a.q = precision >= 0 ? io.q : nullptr;
    a.out = (GradOut *)g->hout_dev;
    a.cnt = (unsigned int *)g->cnt.p;
    hipError_t e = launch_grad_cnn2_fwd(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_cnn2_fwd launch: %s", hipGetErrorString(e));
    ++g->launches;
    e = launch_grad_cnn2_bwd(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_cnn2_bwd launch: %s", hipGetErrorString(e));
    ++g->launches;
    e = launch_grad_cnn2_sum(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_cnn2_sum launch: %s", hipGetErrorString(e));
    ++g->launches;
    e = launch_grad_cnn2_tail(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_cnn2_tail launch: %s", hipGetErrorString(e));
    ++g->launches;
    CHK(grad_finish_call(c, g, io, delta_out, a.q ? q_out : nullptr, loss_out, norm_out));
    drain.armed = false;
    return BK_OK;
}
