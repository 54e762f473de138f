// bk_shares_api.hip -- the host side of bk_shares_* (include/bk.h; the
// kernels: bk_shares.hip; the state: bk_ctx.h struct Shares).
//
// The secure-aggregation path of an iteration (DistSys/main.go:151 SECURE_AGG):
// a client's shares (generateMinerSecretShares, kyber.go:456-482), the miner's
// store of one part per client and its sum over the agreed node list
// (Peer.RegisterSecret main.go:256-286, getSecretShares :2157-2189,
// aggregateSecret kyber.go:244-287), and the leader's recovery
// (recoverAggregateUpdates honest.go:442-502).  Every entry is synchronous: its
// inputs are consumed and its outputs valid on return.  Host inputs are copied
// to a device staging buffer of the context, device inputs are read where they
// are; one kernel launch per generate, sum and recover.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <new>

#include "bk_ctx.h"

namespace bk {

void shares_destroy(Shares *s) {
    if (!s) return;
    for (DevBuf *b : {&s->store, &s->own, &s->slots, &s->in, &s->w, &s->out, &s->bad})
        if (b->p) (void)hipFree(b->p);
    delete s;
}

}  // namespace bk

namespace {

constexpr int64_t SHARES_MAX_D = (int64_t)1 << 30;

// an error path: queued copies may still read the caller's memory
struct Drain {
    hipStream_t st;
    bool armed = true;
    ~Drain() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};

int check_where(int where) {
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    return BK_OK;
}

int check_d(int64_t d) {
    if (d < 1) return fail(BK_EINVAL, "d=%lld < 1", (long long)d);
    if (d > SHARES_MAX_D) return fail(BK_EINVAL, "d=%lld > 2^30", (long long)d);
    return BK_OK;
}

int check_poly(int poly_size) {
    if (poly_size < 1 || poly_size > BK_SHARES_MAX_POLY)
        return fail(BK_EINVAL, "poly_size=%d outside [1, %d]", poly_size, BK_SHARES_MAX_POLY);
    return BK_OK;
}

int check_precision(int precision) {
    if (precision < 0 || precision > 18)
        return fail(BK_EINVAL, "precision=%d outside [0, 18]", precision);
    return BK_OK;
}

// 10^p, exact for p <= 22 (what Go's math.Pow(10, p) returns)
double scale_of(int precision) {
    double s = 1.0;
    for (int i = 0; i < precision; ++i) s *= 10.0;
    return s;
}

int get_shares(bk_ctx *c, Shares **out) {
    if (!c->shares) {
        c->shares = new (std::nothrow) Shares();
        if (!c->shares) return fail(BK_ENOMEM, "host allocation of the share state failed");
    }
    *out = c->shares;
    return BK_OK;
}

int check_live(const bk_ctx *c, const char *who) {
    if (!c->shares || !c->shares->begun) return fail(BK_EINVAL, "%s without bk_shares_begin", who);
    return BK_OK;
}

hipMemcpyKind to_dev(int where) {
    return where == BK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
}

}  // namespace

int64_t bk_shares_chunks(int64_t d, int poly_size) {
    if (check_d(d) != BK_OK || check_poly(poly_size) != BK_OK) return -1;
    return (d + poly_size - 1) / poly_size;
}

int bk_shares_generate(bk_ctx *c, const double *delta, int where, int64_t d, int precision,
                       int poly_size, int total_shares, int64_t *y_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!delta) return fail(BK_EINVAL, "null delta");
    CHK(check_where(where));
    CHK(check_d(d));
    CHK(check_precision(precision));
    CHK(check_poly(poly_size));
    if (total_shares < poly_size || total_shares > BK_SHARES_MAX_POINTS)
        return fail(BK_EINVAL, "total_shares=%d outside [poly_size=%d, %d]", total_shares,
                    poly_size, BK_SHARES_MAX_POINTS);
    if (!y_out) return fail(BK_EINVAL, "null y_out");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    Shares *sh = nullptr;
    CHK(get_shares(c, &sh));
    const hipStream_t st = c->stream;
    const int64_t chunks = (d + poly_size - 1) / poly_size;
    const size_t ybytes = (size_t)chunks * total_shares * 8;
    const double *din = delta;
    int64_t *dy = y_out;
    if (where != BK_DEVICE) {
        CHK(ensure(sh->in, (size_t)d * 8));
        CHK(ensure(sh->out, ybytes));
        din = (const double *)sh->in.p;
        dy = (int64_t *)sh->out.p;
    }
    Drain drain{st};
    ++sh->stats[2];
    if (where != BK_DEVICE) {
        HIPCHK(hipMemcpyAsync(sh->in.p, delta, (size_t)d * 8, hipMemcpyHostToDevice, st));
        ++sh->stats[1];
    }
    const hipError_t e = launch_shares_gen(din, d, scale_of(precision), poly_size, total_shares, dy,
                                           c->shares_gen_per_chunk != 0, st);
    if (e != hipSuccess) return fail(BK_EHIP, "k_shares_gen launch: %s", hipGetErrorString(e));
    ++sh->stats[0];
    if (where != BK_DEVICE) {
        HIPCHK(hipMemcpyAsync(y_out, dy, ybytes, hipMemcpyDeviceToHost, st));
        ++sh->stats[1];
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    return BK_OK;
}

int bk_shares_begin(bk_ctx *c, int64_t d, int poly_size, int held, int64_t n_cap) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_d(d));
    CHK(check_poly(poly_size));
    if (held < 1 || held > BK_SHARES_MAX_POINTS)
        return fail(BK_EINVAL, "held=%d outside [1, %d]", held, BK_SHARES_MAX_POINTS);
    if (n_cap < 1 || n_cap > BK_MAX_N)
        return fail(BK_EINVAL, "n_cap=%lld outside [1, BK_MAX_N=%d]", (long long)n_cap, BK_MAX_N);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    Shares *sh = nullptr;
    CHK(get_shares(c, &sh));
    const int64_t chunks = (d + poly_size - 1) / poly_size;
    const int64_t elems = chunks * held, stride = (elems + 1) / 2 * 2;
    sh->begun = false;  // no store until its buffers exist
    sh->own_valid = false;
    HIPCHK(hipStreamSynchronize(c->stream));
    CHK(ensure(sh->store, (size_t)n_cap * stride * 8));
    CHK(ensure(sh->own, (size_t)stride * 8));
    // the padding word of an odd part is read (never stored) by k_shares_sum
    HIPCHK(hipMemsetAsync(sh->store.p, 0, (size_t)n_cap * stride * 8, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    sh->d = d;
    sh->poly = poly_size;
    sh->held = held;
    sh->chunks = chunks;
    sh->part_elems = elems;
    sh->stride = stride;
    sh->n_cap = n_cap;
    sh->count = 0;
    sh->begun = true;
    return BK_OK;
}

int bk_shares_add(bk_ctx *c, const int64_t *part, int where, int64_t *slot) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!part) return fail(BK_EINVAL, "null part");
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_shares_add"));
    Shares *sh = c->shares;
    if (sh->count >= sh->n_cap)
        return fail(BK_EINVAL, "the store holds its n_cap=%lld parts", (long long)sh->n_cap);
    DeviceGuard dg(c->device);
    Drain drain{c->stream};
    ++sh->stats[2];
    HIPCHK(hipMemcpyAsync((int64_t *)sh->store.p + sh->count * sh->stride, part,
                          (size_t)sh->part_elems * 8, to_dev(where), c->stream));
    ++sh->stats[1];
    HIPCHK(wait_stream(c));
    drain.armed = false;
    if (slot) *slot = sh->count;
    ++sh->count;
    return BK_OK;
}

int bk_shares_count(bk_ctx *c, int64_t *count) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!count) return fail(BK_EINVAL, "null count");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_shares_count"));
    *count = c->shares->count;
    return BK_OK;
}

int bk_shares_sum(bk_ctx *c, const int64_t *slots, int64_t count, int64_t *sum_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!slots) return fail(BK_EINVAL, "null slots");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_shares_sum"));
    Shares *sh = c->shares;
    if (count > sh->count)
        return fail(BK_EINVAL, "count=%lld exceeds the %lld parts held", (long long)count,
                    (long long)sh->count);
    std::vector<bool> seen((size_t)sh->count, false);
    for (int64_t i = 0; i < count; ++i) {
        const int64_t s = slots[i];
        if (s < 0 || s >= sh->count)
            return fail(BK_EINVAL, "slots[%lld]=%lld outside [0, %lld)", (long long)i, (long long)s,
                        (long long)sh->count);
        if (seen[(size_t)s]) return fail(BK_EINVAL, "slot %lld listed twice", (long long)s);
        seen[(size_t)s] = true;
    }
    DeviceGuard dg(c->device);
    CHK(ensure(sh->slots, (size_t)count * 8));
    const hipStream_t st = c->stream;
    Drain drain{st};
    ++sh->stats[2];
    sh->own_valid = false;
    HIPCHK(hipMemcpyAsync(sh->slots.p, slots, (size_t)count * 8, hipMemcpyHostToDevice, st));
    ++sh->stats[1];
    const hipError_t e =
        launch_shares_sum((const int64_t *)sh->store.p, sh->stride, sh->part_elems,
                          (const int64_t *)sh->slots.p, count, (int64_t *)sh->own.p, c->num_cu, st);
    if (e != hipSuccess) return fail(BK_EHIP, "k_shares_sum launch: %s", hipGetErrorString(e));
    ++sh->stats[0];
    if (sum_out) {
        HIPCHK(hipMemcpyAsync(sum_out, sh->own.p, (size_t)sh->part_elems * 8, hipMemcpyDeviceToHost,
                              st));
        ++sh->stats[1];
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    sh->own_valid = true;
    return BK_OK;
}

int bk_shares_recover(bk_ctx *c, const int64_t *const *parts, const int *held, const int64_t *xs,
                      int nparts, int where, int64_t d, int poly_size, int precision,
                      const double *global_w, int64_t *coef_out, double *delta_out,
                      double *global_out, int64_t *bad_chunks) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!parts) return fail(BK_EINVAL, "null parts");
    if (!held) return fail(BK_EINVAL, "null held");
    if (!xs) return fail(BK_EINVAL, "null xs");
    if (nparts < 1 || nparts > BK_SHARES_MAX_POINTS)
        return fail(BK_EINVAL, "nparts=%d outside [1, %d]", nparts, BK_SHARES_MAX_POINTS);
    CHK(check_where(where));
    CHK(check_d(d));
    CHK(check_poly(poly_size));
    CHK(check_precision(precision));
    if (!global_w) return fail(BK_EINVAL, "null global_w");
    if (!global_out) return fail(BK_EINVAL, "null global_out");
    if (!bad_chunks) return fail(BK_EINVAL, "null bad_chunks");
    int S = 0, own = -1;
    for (int i = 0; i < nparts; ++i) {
        if (held[i] < 1 || held[i] > BK_SHARES_MAX_POINTS)
            return fail(BK_EINVAL, "held[%d]=%d outside [1, %d]", i, held[i], BK_SHARES_MAX_POINTS);
        S += held[i];
        if (!parts[i]) {
            if (own >= 0) return fail(BK_EINVAL, "null parts[%d] and parts[%d]: at most one", own, i);
            own = i;
        }
    }
    if (S < poly_size || S > BK_SHARES_MAX_POINTS)
        return fail(BK_EINVAL, "%d points outside [poly_size=%d, %d]", S, poly_size,
                    BK_SHARES_MAX_POINTS);
    // the share points s - 10, s < 64: with |x| <= 53 the recovery's 128-bit
    // intermediates stay below 2^125 (bk_shares.hip)
    for (int s = 0; s < S; ++s) {
        if (xs[s] < -SHARES_X0 || xs[s] >= BK_SHARES_MAX_POINTS - SHARES_X0)
            return fail(BK_EINVAL, "xs[%d]=%lld outside [%d, %d]", s, (long long)xs[s], -SHARES_X0,
                        BK_SHARES_MAX_POINTS - SHARES_X0 - 1);
        for (int t = 0; t < s; ++t)
            if (xs[t] == xs[s]) return fail(BK_EINVAL, "xs[%d] == xs[%d]: the nodes must differ", t, s);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (own >= 0) {
        CHK(check_live(c, "bk_shares_recover (a null part)"));
        const Shares *o = c->shares;
        if (!o->own_valid) return fail(BK_EINVAL, "null parts[%d] without bk_shares_sum", own);
        if (o->d != d || o->poly != poly_size || o->held != held[own])
            return fail(BK_EINVAL,
                        "null parts[%d]: the own aggregate has d=%lld poly_size=%d held=%d", own,
                        (long long)o->d, o->poly, o->held);
    }
    DeviceGuard dg(c->device);
    Shares *sh = nullptr;
    CHK(get_shares(c, &sh));
    const hipStream_t st = c->stream;
    const bool host = where != BK_DEVICE;
    const int64_t chunks = (d + poly_size - 1) / poly_size;
    const size_t db = (size_t)d * 8;
    if (host) {
        CHK(ensure(sh->in, (size_t)chunks * S * 8));
        CHK(ensure(sh->w, db));
        CHK(ensure(sh->out, 3 * db));
    }
    CHK(ensure(sh->bad, 8));
    Drain drain{st};
    ++sh->stats[2];
    SharesPoints pts = {};
    int64_t *stage = (int64_t *)sh->in.p;
    int s = 0;
    for (int i = 0; i < nparts; ++i) {
        const int64_t *base = parts[i];
        if (i == own) {
            base = (const int64_t *)sh->own.p;
        } else if (host) {
            const size_t bytes = (size_t)chunks * held[i] * 8;
            HIPCHK(hipMemcpyAsync(stage, parts[i], bytes, hipMemcpyHostToDevice, st));
            ++sh->stats[1];
            base = stage;
            stage += chunks * held[i];
        }
        for (int l = 0; l < held[i]; ++l, ++s) {
            pts.base[s] = base + l;
            pts.stride[s] = held[i];
            pts.x[s] = (int)xs[s];
        }
    }
    const double *dw = global_w;
    int64_t *dcoef = coef_out;
    double *ddelta = delta_out, *dglobal = global_out;
    if (host) {
        HIPCHK(hipMemcpyAsync(sh->w.p, global_w, db, hipMemcpyHostToDevice, st));
        ++sh->stats[1];
        dw = (const double *)sh->w.p;
        dcoef = coef_out ? (int64_t *)sh->out.p : nullptr;
        ddelta = delta_out ? (double *)sh->out.p + d : nullptr;
        dglobal = (double *)sh->out.p + 2 * d;
    }
    HIPCHK(hipMemsetAsync(sh->bad.p, 0, 8, st));
    const hipError_t e =
        launch_shares_recover(pts, S, poly_size, d, scale_of(precision), dw, dcoef, ddelta, dglobal,
                              (unsigned long long *)sh->bad.p, st);
    if (e != hipSuccess) return fail(BK_EHIP, "k_shares_recover launch: %s", hipGetErrorString(e));
    ++sh->stats[0];
    if (host) {
        HIPCHK(hipMemcpyAsync(global_out, dglobal, db, hipMemcpyDeviceToHost, st));
        ++sh->stats[1];
        if (coef_out) {
            HIPCHK(hipMemcpyAsync(coef_out, dcoef, db, hipMemcpyDeviceToHost, st));
            ++sh->stats[1];
        }
        if (delta_out) {
            HIPCHK(hipMemcpyAsync(delta_out, ddelta, db, hipMemcpyDeviceToHost, st));
            ++sh->stats[1];
        }
    }
    unsigned long long nbad = 0;
    HIPCHK(hipMemcpyAsync(&nbad, sh->bad.p, 8, hipMemcpyDeviceToHost, st));
    ++sh->stats[1];
    HIPCHK(wait_stream(c));
    drain.armed = false;
    *bad_chunks = (int64_t)nbad;
    sh->stats[3] += (int64_t)nbad;
    return BK_OK;
}

int bk_shares_stats(bk_ctx *c, int64_t out[4]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = 0; i < 4; ++i) out[i] = c->shares ? c->shares->stats[i] : 0;
    return BK_OK;
}
