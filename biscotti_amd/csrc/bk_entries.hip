// bk_entries.hip -- the thin entries of SURVEY.md §8(f): block aggregation, the
// quantised sum, the noise application and both RONI variants (the kernels:
// bk_aggregate.hip, bk_roni.hip).
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "bk_ctx.h"

// ---- block aggregation, quantised sum, noise ------
static int check_rows(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                      int64_t m) {
    CHK(check_common(c, dX, dtype, n, d, ld));
    if (m < 0) return fail(BK_EINVAL, "m=%lld < 0", (long long)m);
    if (m > BK_MAX_N) return fail(BK_ENOTSUP, "m=%lld exceeds BK_MAX_N=%d", (long long)m, BK_MAX_N);
    return BK_OK;
}

int bk_aggregate_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
                        const int64_t *d_idx, int64_t m, double *d_global) {
    CHK(check_rows(c, dX, dtype, n, d, ld, m));
    if (!d_global || (m > 0 && !d_idx)) return fail(BK_EINVAL, "null d_idx / d_global");
    if (m == 0) return BK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return timed(c, BK_K_AGGREGATE, [&] {
        return launch_accumulate(dX, dtype, ld, d, d_idx, (int)m, d_global, c->num_cu, c->stream);
    });
}

int bk_aggregate(bk_ctx *c, const void *X, int where, int dtype, int64_t n, int64_t d, int64_t ld,
                 const int64_t *idx, int64_t m, double *global) {
    CHK(check_rows(c, X, dtype, n, d, ld, m));
    if (!global || (m > 0 && !idx)) return fail(BK_EINVAL, "null idx / global");
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    for (int64_t r = 0; r < m; ++r)
        if (idx[r] < 0 || idx[r] >= n)
            return fail(BK_EINVAL, "idx[%lld]=%lld out of [0,%lld)", (long long)r,
                        (long long)idx[r], (long long)n);
    if (m == 0) return BK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    // on an error return, queued copies may still read X / hidx / global
    HostDrain drain{c};
    const size_t es = esize(dtype);
    const void *dX = X;
    int64_t dld = ld;
    if (where != BK_DEVICE) {
        // only the accepted rows cross PCIe: gather them (in idx order) into the stage
        CHK(ensure(c->X, (size_t)m * d * es));
        char *dst = (char *)c->X.p;
        CHK(timed(c, BK_K_H2D, [&] {
            hipError_t e = hipSuccess;
            for (int64_t r = 0; r < m && e == hipSuccess; ++r)
                e = hipMemcpyAsync(dst + (size_t)r * d * es, (const char *)X + (size_t)idx[r] * ld * es,
                                   (size_t)d * es, hipMemcpyHostToDevice, c->stream);
            return e;
        }));
        dX = dst;
        dld = d;
    }
    CHK(ensure(c->idx, (size_t)m * sizeof(int64_t)));
    CHK(ensure(c->mean, (size_t)d * sizeof(double)));
    int64_t *didx = (int64_t *)c->idx.p;
    double *dglob = (double *)c->mean.p;
    std::vector<int64_t> hidx((size_t)m);
    for (int64_t r = 0; r < m; ++r) hidx[r] = where != BK_DEVICE ? r : idx[r];
    HIPCHK(hipMemcpyAsync(didx, hidx.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipMemcpyAsync(dglob, global, (size_t)d * sizeof(double), hipMemcpyHostToDevice,
                          c->stream));
    CHK(timed(c, BK_K_AGGREGATE, [&] {
        return launch_accumulate(dX, dtype, dld, d, didx, (int)m, dglob, c->num_cu, c->stream);
    }));
    CHK(timed(c, BK_K_D2H, [&] {
        return hipMemcpyAsync(global, dglob, (size_t)d * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream);
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    return BK_OK;
}

int bk_quantized_sum_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d,
                            int64_t ld, const int64_t *d_idx, int64_t m, int precision,
                            int64_t *d_sum, double *d_sum_float) {
    CHK(check_rows(c, dX, dtype, n, d, ld, m));
    if (!d_sum || (m > 0 && !d_idx)) return fail(BK_EINVAL, "null d_idx / d_sum");
    if (precision < 0 || precision > 18)
        return fail(BK_EINVAL, "precision=%d outside [0, 18]", precision);
    double scale = 1.0;  // 10^p, exact for p <= 22 (what Go's math.Pow(10, p) returns)
    for (int i = 0; i < precision; ++i) scale *= 10.0;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return timed(c, BK_K_QSUM, [&] {
        return launch_qsum(dX, dtype, ld, d, d_idx, (int)m, scale, d_sum, d_sum_float, c->num_cu,
                           c->stream);
    });
}

int bk_noise_apply_device(bk_ctx *c, const double *d_delta, int64_t n, int64_t d, int64_t ld,
                          const double *d_noise, int64_t k, int64_t noise_ld, double *d_out,
                          int64_t out_ld) {
    CHK(check_common(c, d_delta, BK_F64, n, d, ld));
    if (!d_out || (k > 0 && !d_noise)) return fail(BK_EINVAL, "null d_noise / d_out");
    if (k < 0) return fail(BK_EINVAL, "k=%lld < 0", (long long)k);
    if (k > 0 && noise_ld < d) return fail(BK_EINVAL, "noise_ld=%lld < d", (long long)noise_ld);
    if (out_ld < d) return fail(BK_EINVAL, "out_ld=%lld < d", (long long)out_ld);
    if (d_out == d_delta && out_ld != ld) return fail(BK_EINVAL, "in-place needs out_ld == ld");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return timed(c, BK_K_NOISE, [&] {
        return launch_noise(d_delta, ld, n, d, d_noise, k, noise_ld, d_out, out_ld, c->num_cu,
                            c->stream);
    });
}

// ---- RONI ------------------------------------------
static int check_roni(int64_t nv, int64_t d, int64_t ldv, int64_t n, int64_t ld) {
    if (nv < 1 || d < 1) return fail(BK_EINVAL, "need nv >= 1 and d >= 1");
    if (ldv < d) return fail(BK_EINVAL, "ldv=%lld < d=%lld", (long long)ldv, (long long)d);
    if (n < 0) return fail(BK_EINVAL, "n=%lld < 0", (long long)n);
    if (n > 0 && ld < d) return fail(BK_EINVAL, "ld=%lld < d=%lld", (long long)ld, (long long)d);
    if (n > 65534) return fail(BK_ENOTSUP, "RONI n=%lld exceeds 65534", (long long)n);
    if (d > ((int64_t)1 << 21)) return fail(BK_ENOTSUP, "RONI d=%lld exceeds 2^21", (long long)d);
    return BK_OK;
}

int bk_roni_device(bk_ctx *c, const double *d_Xv, int64_t nv, int64_t d, int64_t ldv,
                   const double *d_yv, const double *d_ww, const double *d_deltas, int64_t n,
                   int64_t ld, double *d_scores) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_roni(nv, d, ldv, n, ld));
    if (!d_Xv || !d_yv || !d_ww || (n > 0 && (!d_deltas || !d_scores)))
        return fail(BK_EINVAL, "null pointer argument");
    if (n == 0) return BK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(ensure(c->roni_cnt, (size_t)(n + 1) * sizeof(unsigned int)));
    CHK(ensure(c->rmc_ws, roni_ws(n, d)));
    unsigned int *cnt = (unsigned int *)c->roni_cnt.p;
    return timed(c, BK_K_RONI, [&] {
        return launch_roni(d_Xv, nv, d, ldv, d_yv, d_ww, d_deltas, n, ld, (double *)c->rmc_ws.p, cnt,
                           d_scores, c->stream);
    });
}

int bk_roni_set_validation(bk_ctx *c, const double *Xv, int64_t nv, int64_t d, int64_t ldv,
                           const double *yv) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_roni(nv, d, ldv, 0, d));
    if (!Xv || !yv) return fail(BK_EINVAL, "null Xv / yv");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    c->roni_nv = 0;  // invalid until the new set has landed
    c->rr_live = 0;  // a round was evaluated on the old set
    HostDrain drain{c};
    CHK(ensure(c->roni_X, (size_t)nv * d * sizeof(double)));
    CHK(ensure(c->roni_y, (size_t)nv * sizeof(double)));
    HIPCHK(hipMemcpy2DAsync(c->roni_X.p, (size_t)d * sizeof(double), Xv, (size_t)ldv * sizeof(double),
                            (size_t)d * sizeof(double), (size_t)nv, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->roni_y.p, yv, (size_t)nv * sizeof(double), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    c->roni_nv = nv;
    c->roni_dim = d;
    return BK_OK;
}

int bk_roni(bk_ctx *c, const double *ww, const double *deltas, int64_t n, int64_t d, int64_t ld,
            double *scores) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);  // roni_nv / roni_dim change under it
    if (c->roni_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_set_validation");
    if (d != c->roni_dim)
        return fail(BK_EINVAL, "d=%lld != validation set's %lld", (long long)d, (long long)c->roni_dim);
    CHK(check_roni(c->roni_nv, d, d, n, ld));
    if (!ww || (n > 0 && (!deltas || !scores))) return fail(BK_EINVAL, "null pointer argument");
    if (n == 0) return BK_OK;
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: queued H2D copies may still read ww / deltas
    CHK(ensure(c->roni_w, (size_t)d * sizeof(double)));
    CHK(ensure(c->roni_d, (size_t)n * d * sizeof(double)));
    CHK(ensure(c->roni_s, (size_t)n * sizeof(double)));
    CHK(ensure(c->roni_cnt, (size_t)(n + 1) * sizeof(unsigned int)));
    CHK(ensure(c->rmc_ws, roni_ws(n, d)));
    double *dw = (double *)c->roni_w.p, *dd = (double *)c->roni_d.p, *ds = (double *)c->roni_s.p;
    CHK(timed(c, BK_K_H2D, [&] {
        hipError_t e = hipMemcpyAsync(dw, ww, (size_t)d * sizeof(double), hipMemcpyHostToDevice,
                                      c->stream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(dd, (size_t)d * sizeof(double), deltas, (size_t)ld * sizeof(double),
                                 (size_t)d * sizeof(double), (size_t)n, hipMemcpyHostToDevice,
                                 c->stream);
        return e;
    }));
    CHK(timed(c, BK_K_RONI, [&] {
        return launch_roni((const double *)c->roni_X.p, c->roni_nv, d, d,
                           (const double *)c->roni_y.p, dw, dd, n, d, (double *)c->rmc_ws.p,
                           (unsigned int *)c->roni_cnt.p, ds, c->stream);
    }));
    CHK(timed(c, BK_K_D2H, [&] {
        return hipMemcpyAsync(scores, ds, (size_t)n * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream);
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    return BK_OK;
}

// ---- SURVEY.md §8(f) row 4, the torch path: the softmax-model RONI --------
static int check_roni_softmax(int64_t nv, int64_t din, int64_t ldv, int64_t C, int64_t n,
                              int64_t ld) {
    if (nv < 1 || din < 1) return fail(BK_EINVAL, "need nv >= 1 and d_in >= 1");
    if (ldv < din) return fail(BK_EINVAL, "ldv=%lld < d_in=%lld", (long long)ldv, (long long)din);
    if (C < 2 || C > 16) return fail(BK_ENOTSUP, "n_classes=%lld outside [2, 16]", (long long)C);
    if (n < 0) return fail(BK_EINVAL, "n=%lld < 0", (long long)n);
    if (n > 0 && ld < C * (din + 1))
        return fail(BK_EINVAL, "ld=%lld < n_classes * (d_in + 1) = %lld", (long long)ld,
                    (long long)(C * (din + 1)));
    if (n > 262139) return fail(BK_ENOTSUP, "RONI n=%lld exceeds 262139", (long long)n);
    if (nv > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "RONI nv=%lld too large", (long long)nv);
    if (din > ((int64_t)1 << 21)) return fail(BK_ENOTSUP, "RONI d_in=%lld exceeds 2^21", (long long)din);
    return BK_OK;
}

int bk_roni_softmax_device(bk_ctx *c, const float *d_Xv, int64_t nv, int64_t d_in, int64_t ldv,
                           const int32_t *d_yv, int64_t n_classes, const double *d_ww,
                           const double *d_deltas, int64_t n, int64_t ld, double *d_scores,
                           int32_t *d_near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_roni_softmax(nv, d_in, ldv, n_classes, n, ld));
    if (!d_Xv || !d_yv || !d_ww || (n > 0 && (!d_deltas || !d_scores)))
        return fail(BK_EINVAL, "null pointer argument");
    if (n == 0) return BK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(ensure(c->rmc_ws, roni_softmax_ws(n, d_in, nv, (int)n_classes)));
    CHK(ensure(c->roni_cnt, (size_t)2 * (n + 1) * sizeof(unsigned int)));
    return timed(c, BK_K_RONI, [&] {
        return launch_roni_softmax(d_Xv, nv, d_in, ldv, d_yv, (int)n_classes, d_ww, d_deltas, n,
                                   ld, (double *)c->rmc_ws.p, nullptr, (unsigned int *)c->roni_cnt.p,
                                   d_scores, d_near_ties, c->stream);
    });
}

int bk_roni_softmax_batches_device(bk_ctx *c, const float *d_Xv, int64_t nv, int64_t d_in,
                                   int64_t ldv, const int32_t *d_yv, int64_t n_classes,
                                   const double *d_ww, const double *d_deltas, int64_t n,
                                   int64_t ld, const int64_t *d_idx, int64_t nb, double *d_scores,
                                   int32_t *d_near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_roni_softmax(nv, d_in, ldv, n_classes, n, ld));
    if (nb < 1) return fail(BK_EINVAL, "need a batch of nb >= 1 samples (nb=%lld)", (long long)nb);
    if (n > 0x7fffffff) return fail(BK_ENOTSUP, "RONI n=%lld exceeds the grid", (long long)n);
    if (!d_Xv || !d_yv || !d_ww || (n > 0 && (!d_deltas || !d_scores || !d_idx)))
        return fail(BK_EINVAL, "null pointer argument");
    if (n == 0) return BK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    return timed(c, BK_K_RONI, [&] {
        return launch_roni_softmax_batches(d_Xv, nv, d_in, ldv, d_yv, (int)n_classes, d_ww,
                                           d_deltas, n, ld, d_idx, nb, d_scores, d_near_ties,
                                           c->stream);
    });
}

int bk_roni_softmax_set_validation(bk_ctx *c, const float *Xv, int64_t nv, int64_t d_in,
                                   int64_t ldv, const int32_t *yv, int64_t n_classes) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_roni_softmax(nv, d_in, ldv, n_classes, 0, 0));
    if (!Xv || !yv) return fail(BK_EINVAL, "null Xv / yv");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    c->rmc_nv = 0;  // invalid until the new set has landed
    c->rs_live = 0;  // a round was evaluated on the old set
    HostDrain drain{c};
    CHK(ensure(c->rmc_X, (size_t)nv * d_in * sizeof(float)));
    CHK(ensure(c->rmc_y, (size_t)nv * sizeof(int32_t)));
    CHK(ensure(c->rmc_xn, (size_t)nv * sizeof(double)));
    HIPCHK(hipMemcpy2DAsync(c->rmc_X.p, (size_t)d_in * sizeof(float), Xv, (size_t)ldv * sizeof(float),
                            (size_t)d_in * sizeof(float), (size_t)nv, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->rmc_y.p, yv, (size_t)nv * sizeof(int32_t), hipMemcpyHostToDevice,
                          c->stream));
    // the samples' norms (the near-tie bound), once per validation set
    HIPCHK(launch_roni_xnorm((const float *)c->rmc_X.p, nv, d_in, d_in, (double *)c->rmc_xn.p,
                             c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    c->rmc_nv = nv;
    c->rmc_din = d_in;
    c->rmc_C = n_classes;
    return BK_OK;
}

// the host forms: ww / deltas (and the batches' indices) to the device, K8,
// scores and near-tie counts back; synchronous
static int roni_softmax_host(bk_ctx *c, const double *ww, const double *deltas, int64_t n,
                             int64_t ld, const int64_t *idx, int64_t nb, double *scores,
                             int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->rmc_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_softmax_set_validation");
    const int64_t nv = c->rmc_nv, din = c->rmc_din, C = c->rmc_C, d = C * (din + 1);
    CHK(check_roni_softmax(nv, din, din, C, n, ld));
    if (!ww || (n > 0 && (!deltas || !scores))) return fail(BK_EINVAL, "null pointer argument");
    if (idx) {
        if (nb < 1) return fail(BK_EINVAL, "need a batch of nb >= 1 samples (nb=%lld)", (long long)nb);
        if (n > 0x7fffffff) return fail(BK_ENOTSUP, "RONI n=%lld exceeds the grid", (long long)n);
        for (int64_t i = 0; i < 2 * n * nb; ++i)
            if (idx[i] < 0 || idx[i] >= nv)
                return fail(BK_EINVAL, "batch index %lld = %lld outside [0, %lld)", (long long)i,
                            (long long)idx[i], (long long)nv);
    }
    if (n == 0) return BK_OK;
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: queued H2D copies may still read ww / deltas
    const int64_t nnt = idx ? 2 * n : n + 1;
    CHK(ensure(c->roni_w, (size_t)d * sizeof(double)));
    CHK(ensure(c->roni_d, (size_t)n * d * sizeof(double)));
    CHK(ensure(c->roni_s, (size_t)n * sizeof(double)));
    CHK(ensure(c->rmc_nt, (size_t)nnt * sizeof(int32_t)));
    if (idx) CHK(ensure(c->rmc_idx, (size_t)2 * n * nb * sizeof(int64_t)));
    if (!idx) {
        CHK(ensure(c->rmc_ws, roni_softmax_ws(n, din, nv, (int)C)));
        CHK(ensure(c->roni_cnt, (size_t)2 * (n + 1) * sizeof(unsigned int)));
    }
    double *dw = (double *)c->roni_w.p, *dd = (double *)c->roni_d.p, *ds = (double *)c->roni_s.p;
    int32_t *dnt = (int32_t *)c->rmc_nt.p;
    CHK(timed(c, BK_K_H2D, [&] {
        hipError_t e = hipMemcpyAsync(dw, ww, (size_t)d * sizeof(double), hipMemcpyHostToDevice,
                                      c->stream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(dd, (size_t)d * sizeof(double), deltas, (size_t)ld * sizeof(double),
                                 (size_t)d * sizeof(double), (size_t)n, hipMemcpyHostToDevice,
                                 c->stream);
        if (e == hipSuccess && idx)
            e = hipMemcpyAsync(c->rmc_idx.p, idx, (size_t)2 * n * nb * sizeof(int64_t),
                               hipMemcpyHostToDevice, c->stream);
        return e;
    }));
    CHK(timed(c, BK_K_RONI, [&] {
        if (idx)
            return launch_roni_softmax_batches((const float *)c->rmc_X.p, nv, din, din,
                                               (const int32_t *)c->rmc_y.p, (int)C, dw, dd, n, d,
                                               (const int64_t *)c->rmc_idx.p, nb, ds, dnt,
                                               c->stream);
        return launch_roni_softmax((const float *)c->rmc_X.p, nv, din, din,
                                   (const int32_t *)c->rmc_y.p, (int)C, dw, dd, n, d,
                                   (double *)c->rmc_ws.p, (const double *)c->rmc_xn.p,
                                   (unsigned int *)c->roni_cnt.p, ds, dnt, c->stream);
    }));
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(scores, ds, (size_t)n * sizeof(double), hipMemcpyDeviceToHost,
                                      c->stream);
        if (e == hipSuccess && near_ties)
            e = hipMemcpyAsync(near_ties, dnt, (size_t)nnt * sizeof(int32_t),
                               hipMemcpyDeviceToHost, c->stream);
        return e;
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    return BK_OK;
}

// ---- RONI rounds: the model of one iteration held with its evaluation done --
static int check_where(int where) {
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    return BK_OK;
}

// a begin's upload: ww is consumed on return, the evaluation behind it runs on
static int round_upload_ww(bk_ctx *c, DevBuf &w, const double *ww, int64_t d, int where) {
    CHK(ensure(w, (size_t)d * sizeof(double)));
    if (!c->ev_round) HIPCHK(hipEventCreateWithFlags(&c->ev_round, hipEventDisableTiming));
    CHK(timed(c, BK_K_H2D, [&] {
        return hipMemcpyAsync(w.p, ww, (size_t)d * sizeof(double),
                              where == BK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              c->stream);
    }));
    HIPCHK(hipEventRecord(c->ev_round, c->stream));
    HIPCHK(hipEventSynchronize(c->ev_round));
    return BK_OK;
}

// the mapped pinned block a score call's kernels write: count scores, then
// nnt near-tie counts (1 + count; the mini-batch form: 2 count)
static int ensure_round_out(bk_ctx *c, int64_t count, int64_t nnt) {
    const size_t bytes = (size_t)count * sizeof(double) + (size_t)nnt * sizeof(int32_t);
    if (bytes <= c->round_out_bytes) return BK_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->round_out) (void)hipHostFree(c->round_out);
    c->round_out = c->round_out_dev = nullptr;
    c->round_out_bytes = 0;
    const size_t want = bytes < 4096 ? 4096 : bytes;
    HIPCHK(hipHostMalloc(&c->round_out, want,
                         hipHostMallocPortable | hipHostMallocMapped | hipHostMallocNonCoherent));
    HIPCHK(hipHostGetDevicePointer(&c->round_out_dev, c->round_out, 0));
    c->round_out_bytes = want;
    return BK_OK;
}

// A score call past its checks (the context mutex held): host rows staged on
// the device (device rows are read where they are), the groups' counters
// zeroed (cnt_words each), one launch per group of up to RONI_ROUND_G rows, one
// wait, then host memcpys out of the mapped block (count scores, nnt near-tie
// counts).  launch(rows, g, q0, cnt, scores, near): the group of rows q0 ..
// q0 + g, its counters, and the block's score and near-tie (nullable) arrays
template <typename F>
static int round_score(bk_ctx *c, int kid, const double *const *deltas, int64_t count, int where,
                       int64_t d, double *scores, int32_t *near_ties, int64_t nnt, int cnt_words,
                       F &&launch) {
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: queued copies and launches may still read the rows
    const int64_t groups = (count + RONI_ROUND_G - 1) / RONI_ROUND_G;
    const size_t cbytes = (size_t)groups * cnt_words * sizeof(unsigned int);
    CHK(ensure(c->round_cnt, cbytes));
    CHK(ensure_round_out(c, count, nnt));
    const double *staged = nullptr;
    if (where != BK_DEVICE) {
        CHK(ensure(c->round_rows, (size_t)count * d * sizeof(double)));
        double *dst = (double *)c->round_rows.p;
        CHK(timed(c, BK_K_H2D, [&] {
            hipError_t e = hipSuccess;
            for (int64_t i = 0; i < count && e == hipSuccess; ++i)
                e = hipMemcpyAsync(dst + i * d, deltas[i], (size_t)d * sizeof(double),
                                   hipMemcpyHostToDevice, c->stream);
            return e;
        }));
        staged = dst;
    }
    HIPCHK(hipMemsetAsync(c->round_cnt.p, 0, cbytes, c->stream));
    double *dsc = (double *)c->round_out_dev;
    int32_t *dnt = near_ties ? (int32_t *)(dsc + count) : nullptr;
    for (int64_t q0 = 0; q0 < count; q0 += RONI_ROUND_G) {
        const int g = (int)(count - q0 < RONI_ROUND_G ? count - q0 : RONI_ROUND_G);
        RoundRows rows = {};
        for (int q = 0; q < g; ++q) rows.p[q] = staged ? staged + (q0 + q) * d : deltas[q0 + q];
        unsigned int *cnt = (unsigned int *)c->round_cnt.p + q0 / RONI_ROUND_G * cnt_words;
        CHK(timed(c, kid, [&] { return launch(rows, g, q0, cnt, dsc, dnt); }));
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    const char *h = (const char *)c->round_out;
    memcpy(scores, h, (size_t)count * sizeof(double));
    if (near_ties) memcpy(near_ties, h + (size_t)count * sizeof(double), (size_t)nnt * sizeof(int32_t));
    return BK_OK;
}

static int check_round_rows(const double *const *deltas, int64_t count, const double *scores) {
    if (!deltas || !scores) return fail(BK_EINVAL, "null pointer argument");
    for (int64_t i = 0; i < count; ++i)
        if (!deltas[i]) return fail(BK_EINVAL, "null row deltas[%lld]", (long long)i);
    return BK_OK;
}

int bk_roni_round_begin(bk_ctx *c, const double *ww, int64_t d, int where) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->roni_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_set_validation");
    if (d != c->roni_dim)
        return fail(BK_EINVAL, "d=%lld != validation set's %lld", (long long)d, (long long)c->roni_dim);
    CHK(check_roni(c->roni_nv, d, d, 0, d));
    if (!ww) return fail(BK_EINVAL, "null pointer argument");
    CHK(check_where(where));
    DeviceGuard dg(c->device);
    HostDrain drain{c};
    c->rr_live = 0;  // no round until the new one's evaluation is queued
    CHK(ensure(c->rr_base, sizeof(unsigned int)));
    CHK(ensure(c->rr_ws, roni_ws(0, d)));
    CHK(round_upload_ww(c, c->rr_w, ww, d, where));
    // K7 with no new model: model 0's count, bitwise the batched call's
    const double *dw = (const double *)c->rr_w.p;
    CHK(timed(c, BK_K_RONI, [&] {
        return launch_roni((const double *)c->roni_X.p, c->roni_nv, d, d, (const double *)c->roni_y.p,
                           dw, dw, 0, d, (double *)c->rr_ws.p, (unsigned int *)c->rr_base.p, nullptr,
                           c->stream);
    }));
    drain.armed = false;
    c->rr_live = 1;
    return BK_OK;
}

int bk_roni_round_score(bk_ctx *c, const double *const *deltas, int64_t count, int where,
                        double *scores) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->roni_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_set_validation");
    if (!c->rr_live) return fail(BK_EINVAL, "no round: call bk_roni_round_begin");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    const int64_t nv = c->roni_nv, d = c->roni_dim;
    CHK(check_roni(nv, d, d, count, d));
    CHK(check_round_rows(deltas, count, scores));
    CHK(check_where(where));
    return round_score(c, BK_K_RONI_ROUND, deltas, count, where, d, scores, nullptr, 0,
                       ROUND_CNT_WORDS,
                       [&](const RoundRows &rows, int g, int64_t q0, unsigned int *cnt, double *sc,
                           int32_t *) {
                           return launch_roni_round((const double *)c->roni_X.p, nv, d, d,
                                                    (const double *)c->roni_y.p,
                                                    (const double *)c->rr_w.p, rows, g, cnt,
                                                    (const unsigned int *)c->rr_base.p, sc + q0,
                                                    c->stream);
                       });
}

int bk_roni_softmax_round_begin(bk_ctx *c, const double *ww, int where) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->rmc_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_softmax_set_validation");
    const int64_t nv = c->rmc_nv, din = c->rmc_din, C = c->rmc_C, d = C * (din + 1);
    CHK(check_roni_softmax(nv, din, din, C, 0, 0));
    if (!ww) return fail(BK_EINVAL, "null pointer argument");
    CHK(check_where(where));
    DeviceGuard dg(c->device);
    HostDrain drain{c};
    c->rs_live = 0;
    CHK(ensure(c->rs_base, 2 * sizeof(unsigned int)));
    CHK(ensure(c->rs_ws, roni_softmax_ws(0, din, nv, (int)C)));
    CHK(round_upload_ww(c, c->rs_w, ww, d, where));
    // K8 with no new model: model 0's correct and near-tie counts, bitwise the
    // batched call's; its widened columns and their norms stay in rs_ws
    const double *dw = (const double *)c->rs_w.p;
    CHK(timed(c, BK_K_RONI, [&] {
        return launch_roni_softmax((const float *)c->rmc_X.p, nv, din, din, (const int32_t *)c->rmc_y.p,
                                   (int)C, dw, dw, 0, d, (double *)c->rs_ws.p,
                                   (const double *)c->rmc_xn.p, (unsigned int *)c->rs_base.p, nullptr,
                                   nullptr, c->stream);
    }));
    drain.armed = false;
    c->rs_live = 1;
    return BK_OK;
}

int bk_roni_softmax_round_score(bk_ctx *c, const double *const *deltas, int64_t count, int where,
                                double *scores, int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->rmc_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_softmax_set_validation");
    if (!c->rs_live) return fail(BK_EINVAL, "no round: call bk_roni_softmax_round_begin");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    const int64_t nv = c->rmc_nv, din = c->rmc_din, C = c->rmc_C, d = C * (din + 1);
    CHK(check_roni_softmax(nv, din, din, C, count, d));
    CHK(check_round_rows(deltas, count, scores));
    CHK(check_where(where));
    return round_score(c, BK_K_RONI_ROUND_SM, deltas, count, where, d, scores, near_ties, count + 1,
                       ROUND_CNT_WORDS,
                       [&](const RoundRows &rows, int g, int64_t q0, unsigned int *cnt, double *sc,
                           int32_t *nt) {
                           return launch_roni_softmax_round(
                               (const float *)c->rmc_X.p, nv, din, din, (const int32_t *)c->rmc_y.p,
                               (int)C, (const double *)c->rs_w.p, rows, g,
                               (const double *)c->rmc_xn.p, cnt, (const unsigned int *)c->rs_base.p,
                               sc + q0, nt ? nt + q0 : nullptr, q0 == 0 ? 1 : 0, c->stream);
                       });
}

// The mini-batch form on the same round (bk_roni_softmax_batches' semantics):
// every check before any copy, launch or state change.  A group's indices ride
// in its launch's arguments when there are at most ROUND_IDX_ARGS of them (the
// verifier's 2 x 10); else all of the call's go up once, as int32, through the
// ragged calls' pinned ring (its slot's event guards the staging bytes)
int bk_roni_softmax_round_score_batches(bk_ctx *c, const double *const *deltas, int64_t count,
                                        int where, const int64_t *idx, int64_t nb, double *scores,
                                        int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!deltas || !idx || !scores) return fail(BK_EINVAL, "null pointer argument");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    if (nb < 1) return fail(BK_EINVAL, "need a batch of nb >= 1 samples (nb=%lld)", (long long)nb);
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->rmc_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_softmax_set_validation");
    if (!c->rs_live) return fail(BK_EINVAL, "no round: call bk_roni_softmax_round_begin");
    const int64_t nv = c->rmc_nv, din = c->rmc_din, C = c->rmc_C, d = C * (din + 1);
    CHK(check_roni_softmax(nv, din, din, C, count, d));
    CHK(check_round_rows(deltas, count, scores));
    for (int64_t j = 0; j < count; ++j)
        for (int e = 0; e < 2; ++e)
            for (int64_t s = 0; s < nb; ++s) {
                const int64_t v = idx[(2 * j + e) * nb + s];
                if (v < 0 || v >= nv)
                    return fail(BK_EINVAL,
                                "batch index %lld outside [0, %lld): update %lld, evaluation %d "
                                "(%s), position %lld",
                                (long long)v, (long long)nv, (long long)j, e,
                                e ? "after" : "original", (long long)s);
            }
    DeviceGuard dg(c->device);
    const int64_t g0 = count < RONI_ROUND_G ? count : RONI_ROUND_G;  // the largest group
    const int32_t *didx = nullptr;
    if (2 * g0 * nb > ROUND_IDX_ARGS) {
        const int64_t total = 2 * count * nb;
        const size_t bytes = (size_t)total * sizeof(int32_t);
        CHK(ensure(c->round_idx, bytes));
        int slot = 0;
        CHK(ragged_stage_slot(c, bytes, &slot));
        int32_t *hs = (int32_t *)c->ragged_stage[slot];
        for (int64_t i = 0; i < total; ++i) hs[i] = (int32_t)idx[i];
        CHK(timed(c, BK_K_H2D, [&] {
            return hipMemcpyAsync(c->round_idx.p, hs, bytes, hipMemcpyHostToDevice, c->stream);
        }));
        HIPCHK(hipEventRecord(c->ev_ragged[slot], c->stream));
        c->ragged_used[slot] = true;
        didx = (const int32_t *)c->round_idx.p;
    }
    return round_score(c, BK_K_RONI_ROUND_SM, deltas, count, where, d, scores, near_ties, 2 * count,
                       ROUND_BATCH_CNT_WORDS,
                       [&](const RoundRows &rows, int g, int64_t q0, unsigned int *cnt, double *sc,
                           int32_t *nt) {
                           RoundIdx ia = {};
                           const bool in_args = 2 * g * nb <= ROUND_IDX_ARGS;
                           if (in_args)
                               for (int64_t i = 0; i < 2 * g * nb; ++i)
                                   ia.v[i] = (int32_t)idx[2 * q0 * nb + i];
                           return launch_roni_softmax_round_batch(
                               (const float *)c->rmc_X.p, nv, din, din, (const int32_t *)c->rmc_y.p,
                               (int)C, (const double *)c->rs_w.p, rows, g,
                               in_args ? nullptr : didx + 2 * q0 * nb, ia, nb, cnt, sc + q0,
                               nt ? nt + 2 * q0 : nullptr, c->stream);
                       });
}

int bk_roni_softmax(bk_ctx *c, const double *ww, const double *deltas, int64_t n, int64_t ld,
                    double *scores, int32_t *near_ties) {
    return roni_softmax_host(c, ww, deltas, n, ld, nullptr, 0, scores, near_ties);
}

int bk_roni_softmax_batches(bk_ctx *c, const double *ww, const double *deltas, int64_t n,
                            int64_t ld, const int64_t *idx, int64_t nb, double *scores,
                            int32_t *near_ties) {
    if (!idx && n > 0) return fail(BK_EINVAL, "null batch indices");
    return roni_softmax_host(c, ww, deltas, n, ld, idx, nb, scores, near_ties);
}
