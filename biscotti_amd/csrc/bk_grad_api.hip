// bk_grad_api.hip -- the host side of bk_grad_* (include/bk.h; the kernels:
// bk_grad.hip; the state: bk_ctx.h struct Grad).
//
// A peer's gradient step (computeUpdate -> oneGradientStep, DistSys/
// honest.go:165-200, 284-324) on its resident shard: one launch for the
// logistic model, two for the softmax model.  Every entry is synchronous.  The
// model, the noise and the outputs share one `where`: host ones are copied to
// and from buffers of the context, except that host outputs of up to
// GRAD_MAPPED_MAX entries are stored by the kernel into a mapped pinned block
// (bk_block_finish's measured cut); device ones are used where they are.  The
// batch's row numbers always come from the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <mutex>
#include <new>

#include "bk_ctx.h"

namespace bk {

void grad_destroy(Grad *g) {
    if (!g) return;
    for (DevBuf *b : {&g->X, &g->y, &g->w, &g->noise, &g->idx, &g->R, &g->part, &g->lossp, &g->out,
                      &g->cnt})
        if (b->p) (void)hipFree(b->p);
    if (g->hout) (void)hipHostFree(g->hout);
    delete g;
}

}  // namespace bk

namespace {

constexpr size_t GRAD_HOUT_HEAD = 64;  // GradOut, padded
constexpr size_t GRAD_HOUT_BYTES = GRAD_HOUT_HEAD + 2 * (size_t)GRAD_MAPPED_MAX * 8;

int grad_state(bk_ctx *c) {
    if (c->grad) return BK_OK;
    c->grad = new (std::nothrow) Grad();
    if (!c->grad) return fail(BK_ENOMEM, "host allocation of the training set failed");
    return BK_OK;
}

int check_set_shape(int64_t nn, int64_t d, int64_t ldx) {
    if (nn < 1 || d < 1)
        return fail(BK_EINVAL, "need nn >= 1 and d >= 1 (nn=%lld, d=%lld)", (long long)nn, (long long)d);
    if (ldx < d) return fail(BK_EINVAL, "ldx=%lld < d=%lld", (long long)ldx, (long long)d);
    return BK_OK;
}

// 10^p, exact for p <= 22 (what Go's math.Pow(10, p) returns)
double scale_of(int precision) {
    double s = 1.0;
    for (int i = 0; i < precision; ++i) s *= 10.0;
    return s;
}

// checks 1 and 2 of a gradient call: no context field is read
int check_call(const bk_ctx *c, const double *ww, int where, int precision, const double *delta_out,
               const int64_t *q_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!ww) return fail(BK_EINVAL, "null ww");
    if (!delta_out) return fail(BK_EINVAL, "null delta_out");
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    if (precision > 18) return fail(BK_EINVAL, "precision=%d exceeds 18", precision);
    if (precision < 0 && q_out) return fail(BK_EINVAL, "q_out without a precision (precision=%d)", precision);
    return BK_OK;
}

// checks 4 to 7, under the context mutex; *n: the batch's rows
int check_batch(const bk_ctx *c, int kind, const int64_t *idx, int64_t count, int64_t *n) {
    const Grad *g = c->grad;
    if (!g || g->kind == EVAL_EMPTY)
        return fail(BK_EINVAL, "no resident training set: call bk_grad_set_*");
    if (g->kind != kind)
        return fail(BK_EINVAL, "the resident training set is a %s one",
                    g->kind == EVAL_SOFTMAX ? "softmax" : "logistic");
    if (idx && count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    if (idx)
        for (int64_t i = 0; i < count; ++i)
            if (idx[i] < 0 || idx[i] >= g->nn)
                return fail(BK_EINVAL, "idx[%lld]=%lld outside [0, %lld)", (long long)i,
                            (long long)idx[i], (long long)g->nn);
    *n = idx ? count : g->nn;
    if (*n > GRAD_MAX_BATCH)
        return fail(BK_ENOTSUP, "a batch of %lld rows exceeds %lld", (long long)*n,
                    (long long)GRAD_MAX_BATCH);
    return BK_OK;
}

// the exit counter (zeroed once: every launch leaves it zero) and the mapped
// block the last workgroup writes
int ensure_out(bk_ctx *c, Grad *g) {
    if (!g->cnt.p) {
        CHK(ensure(g->cnt, 64));
        HIPCHK(hipMemsetAsync(g->cnt.p, 0, 64, c->stream));
    }
    if (!g->hout) {
        void *h = nullptr, *d = nullptr;
        HIPCHK(hipHostMalloc(&h, GRAD_HOUT_BYTES,
                             hipHostMallocPortable | hipHostMallocMapped | hipHostMallocNonCoherent));
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return fail(BK_EHIP, "hipHostGetDevicePointer failed for the gradient block");
        }
        g->hout = (char *)h;
        g->hout_dev = (char *)d;
    }
    return BK_OK;
}

// where a call's kernels read and write
struct GradIO {
    const double *ww = nullptr, *noise = nullptr;
    const int64_t *rows = nullptr;
    double *delta = nullptr;
    int64_t *q = nullptr;
    bool mapped = false, copied = false;
};

int stage_call(bk_ctx *c, Grad *g, const double *ww, int where, const int64_t *idx, int64_t n,
               const double *noise, double *delta_out, int64_t *q_out, GradIO *io) {
    const size_t db = (size_t)g->d * 8;
    const hipStream_t st = c->stream;
    CHK(ensure_out(c, g));
    io->ww = ww;
    io->noise = noise;
    io->delta = delta_out;
    io->q = q_out;
    if (idx) {
        CHK(ensure(g->idx, (size_t)n * 8));
        HIPCHK(hipMemcpyAsync(g->idx.p, idx, (size_t)n * 8, hipMemcpyHostToDevice, st));
        io->rows = (const int64_t *)g->idx.p;
    }
    if (where == BK_DEVICE) return BK_OK;
    CHK(ensure(g->w, db));
    HIPCHK(hipMemcpyAsync(g->w.p, ww, db, hipMemcpyHostToDevice, st));
    io->ww = (const double *)g->w.p;
    if (noise) {
        CHK(ensure(g->noise, db));
        HIPCHK(hipMemcpyAsync(g->noise.p, noise, db, hipMemcpyHostToDevice, st));
        io->noise = (const double *)g->noise.p;
    }
    if (g->d <= GRAD_MAPPED_MAX) {
        io->mapped = true;
        io->delta = (double *)(g->hout_dev + GRAD_HOUT_HEAD);
        io->q = q_out ? (int64_t *)(g->hout_dev + GRAD_HOUT_HEAD) + GRAD_MAPPED_MAX : nullptr;
    } else {
        io->copied = true;
        CHK(ensure(g->out, 2 * db));
        io->delta = (double *)g->out.p;
        io->q = q_out ? (int64_t *)g->out.p + g->d : nullptr;
    }
    return BK_OK;
}

// behind the launches: the outputs' way back, the wait, the scalars
int finish_call(bk_ctx *c, Grad *g, const GradIO &io, double *delta_out, int64_t *q_out,
                double *loss_out, double *norm_out) {
    const size_t db = (size_t)g->d * 8;
    if (io.copied) {
        HIPCHK(hipMemcpyAsync(delta_out, io.delta, db, hipMemcpyDeviceToHost, c->stream));
        if (q_out) HIPCHK(hipMemcpyAsync(q_out, io.q, db, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(wait_stream(c));
    if (io.mapped) {
        memcpy(delta_out, g->hout + GRAD_HOUT_HEAD, db);
        if (q_out) memcpy(q_out, g->hout + GRAD_HOUT_HEAD + (size_t)GRAD_MAPPED_MAX * 8, db);
    }
    const GradOut *o = (const GradOut *)g->hout;
    if (loss_out) *loss_out = o->loss;
    if (norm_out) *norm_out = o->norm;
    ++g->calls;
    return BK_OK;
}

}  // namespace

int bk_grad_set_logistic(bk_ctx *c, const double *X, int64_t nn, int64_t d, int64_t ldx,
                         const double *y) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_shape(nn, d, ldx));
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    if (nn > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "nn=%lld too large", (long long)nn);
    if (d > GRAD_MAX_D) return fail(BK_ENOTSUP, "d=%lld exceeds %lld", (long long)d, (long long)GRAD_MAX_D);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(grad_state(c));
    Grad *g = c->grad;
    g->kind = EVAL_EMPTY;  // empty until the new set has landed
    HostDrain drain{c};
    CHK(ensure(g->X, (size_t)nn * d * sizeof(double)));
    CHK(ensure(g->y, (size_t)nn * sizeof(double)));
    HIPCHK(hipMemcpy2DAsync(g->X.p, (size_t)d * sizeof(double), X, (size_t)ldx * sizeof(double),
                            (size_t)d * sizeof(double), (size_t)nn, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->y.p, y, (size_t)nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    g->nn = nn;
    g->d = d;
    g->din = g->C = 0;
    g->kind = EVAL_LOGISTIC;
    return BK_OK;
}

int bk_grad_set_softmax(bk_ctx *c, const float *X, int64_t nn, int64_t d_in, int64_t ldx,
                        const int32_t *y, int64_t n_classes) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_shape(nn, d_in, ldx));
    if (n_classes < 2) return fail(BK_EINVAL, "n_classes=%lld < 2", (long long)n_classes);
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    for (int64_t i = 0; i < nn; ++i)
        if (y[i] < 0 || y[i] >= n_classes)
            return fail(BK_EINVAL, "label y[%lld]=%d outside [0, %lld)", (long long)i, (int)y[i],
                        (long long)n_classes);
    if (nn > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "nn=%lld too large", (long long)nn);
    if (n_classes > 16) return fail(BK_ENOTSUP, "n_classes=%lld exceeds 16", (long long)n_classes);
    if (d_in > GRAD_MAX_D)
        return fail(BK_ENOTSUP, "d_in=%lld exceeds %lld", (long long)d_in, (long long)GRAD_MAX_D);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(grad_state(c));
    Grad *g = c->grad;
    g->kind = EVAL_EMPTY;
    HostDrain drain{c};
    CHK(ensure(g->X, (size_t)nn * d_in * sizeof(float)));
    CHK(ensure(g->y, (size_t)nn * sizeof(int32_t)));
    HIPCHK(hipMemcpy2DAsync(g->X.p, (size_t)d_in * sizeof(float), X, (size_t)ldx * sizeof(float),
                            (size_t)d_in * sizeof(float), (size_t)nn, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g->y.p, y, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    g->nn = nn;
    g->din = d_in;
    g->C = n_classes;
    g->d = n_classes * (d_in + 1);
    g->kind = EVAL_SOFTMAX;
    return BK_OK;
}

int bk_grad_clear(bk_ctx *c) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->grad) c->grad->kind = EVAL_EMPTY;  // the buffers stay for the next set
    return BK_OK;
}

int bk_grad_logistic(bk_ctx *c, const double *ww, int where, const int64_t *idx, int64_t count,
                     int64_t batch_size, double alpha, double lammy, const double *noise,
                     int precision, double *delta_out, int64_t *q_out, double *loss_out) {
    CHK(check_call(c, ww, where, precision, delta_out, q_out));
    if (batch_size < 1) return fail(BK_EINVAL, "batch_size=%lld < 1", (long long)batch_size);
    std::lock_guard<std::mutex> lk(c->mu);
    int64_t n = 0;
    CHK(check_batch(c, EVAL_LOGISTIC, idx, count, &n));
    Grad *g = c->grad;
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: the queued copies may still read the caller's memory
    GradIO io;
    CHK(stage_call(c, g, ww, where, idx, n, noise, delta_out, q_out, &io));
    const int64_t tiles = (n + GRAD_TILE - 1) / GRAD_TILE;
    if (tiles > 1) {
        CHK(ensure(g->part, (size_t)tiles * g->d * 8));
        CHK(ensure(g->lossp, (size_t)tiles * 8));
    }
    GradLogistic a = {};
    a.X = (const double *)g->X.p;
    a.y = (const double *)g->y.p;
    a.ww = io.ww;
    a.noise = io.noise;
    a.rows = io.rows;
    a.count = n;
    a.d = g->d;
    a.batch = (double)batch_size;
    a.alpha = alpha;
    a.lammy = lammy;
    a.scale = scale_of(precision);
    a.part = (double *)g->part.p;
    a.lossp = (double *)g->lossp.p;
    a.delta = io.delta;
    a.q = precision >= 0 ? io.q : nullptr;
    a.out = (GradOut *)g->hout_dev;
    a.cnt = (unsigned int *)g->cnt.p;
    const hipError_t e = launch_grad_logistic(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_logistic launch: %s", hipGetErrorString(e));
    ++g->launches;
    CHK(finish_call(c, g, io, delta_out, a.q ? q_out : nullptr, loss_out, nullptr));
    drain.armed = false;
    return BK_OK;
}

int bk_grad_softmax(bk_ctx *c, const double *ww, int where, const int64_t *idx, int64_t count,
                    double max_norm, const double *noise, int precision, double *delta_out,
                    int64_t *q_out, double *loss_out, double *norm_out) {
    CHK(check_call(c, ww, where, precision, delta_out, q_out));
    if (!isfinite(max_norm) || !(max_norm > 0.0))
        return fail(BK_EINVAL, "max_norm=%g is not a positive finite number", max_norm);
    std::lock_guard<std::mutex> lk(c->mu);
    int64_t n = 0;
    CHK(check_batch(c, EVAL_SOFTMAX, idx, count, &n));
    Grad *g = c->grad;
    DeviceGuard dg(c->device);
    HostDrain drain{c};
    GradIO io;
    CHK(stage_call(c, g, ww, where, idx, n, noise, delta_out, q_out, &io));
    CHK(ensure(g->R, (size_t)n * 16 * 8));
    CHK(ensure(g->part, (size_t)g->d * 8));
    CHK(ensure(g->lossp, (size_t)((n + 63) / 64) * 8));
    GradSoftmax a = {};
    a.X = (const float *)g->X.p;
    a.y = (const int32_t *)g->y.p;
    a.ww = io.ww;
    a.noise = io.noise;
    a.rows = io.rows;
    a.count = n;
    a.din = g->din;
    a.C = (int)g->C;
    a.max_norm = max_norm;
    a.scale = scale_of(precision);
    a.R = (double *)g->R.p;
    a.part = (double *)g->part.p;
    a.lossp = (double *)g->lossp.p;
    a.delta = io.delta;
    a.q = precision >= 0 ? io.q : nullptr;
    a.out = (GradOut *)g->hout_dev;
    a.cnt = (unsigned int *)g->cnt.p;
    hipError_t e = launch_grad_softmax_fwd(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_softmax_fwd launch: %s", hipGetErrorString(e));
    ++g->launches;
    e = launch_grad_softmax_bwd(a, c->stream);
    if (e != hipSuccess) return fail(BK_EHIP, "k_grad_softmax_bwd launch: %s", hipGetErrorString(e));
    ++g->launches;
    CHK(finish_call(c, g, io, delta_out, a.q ? q_out : nullptr, loss_out, norm_out));
    drain.armed = false;
    return BK_OK;
}

int bk_grad_stats(bk_ctx *c, int64_t out[2]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    out[0] = c->grad ? c->grad->launches : 0;
    out[1] = c->grad ? c->grad->calls : 0;
    return BK_OK;
}
