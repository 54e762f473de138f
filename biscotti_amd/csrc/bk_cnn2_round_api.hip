// bk_cnn2_round_api.hip -- the CNN2 verifier's rounds (include/bk.h
// bk_roni_cnn2_round_*): bk_cnn_round_api.hip's entries for the
// two-layer model -- the iteration's model held on the device as fp64 with its
// per-sample verdicts over the whole validation set, each update's `original`
// from the held verdicts, its `after` by one forward pass.  The kernel is
// k_cnn2_round (bk_cnn2_round.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "bk_ctx.h"

namespace bk {
namespace {

int check_where(int where) {
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    return BK_OK;
}

// the band height of a launch of `samples` samples: the fewest bands that give
// about two workgroups per CU (bh = 1 for a verifier's 10 samples at lfw, one
// band from 2 x CUs samples on); any bh <= ph2 fits the LDS, ph2 being k_cnn2's
int pick_bh(const bk_ctx *c, const Cnn2Dims &m, int64_t samples) {
    if (c->c2r_band > 0) return c->c2r_band < m.ph2 ? c->c2r_band : m.ph2;
    const int64_t cus = c->num_cu > 0 ? c->num_cu : 256;
    int64_t bands = (2 * cus + samples - 1) / samples;
    bands = bands < 1 ? 1 : bands > m.ph2 ? m.ph2 : bands;
    return (int)((m.ph2 + bands - 1) / bands);
}

// the scratch of a launch of `tiles` tiles and the zeroed counters
int ensure_launch_state(bk_ctx *c, int64_t tiles) {
    const int64_t t = tiles < CNN2_ROUND_TILES ? tiles : CNN2_ROUND_TILES;
    CHK(ensure(c->c2r_scratch, (size_t)t * cnn2_tile_floats(c->c2_dims) * sizeof(float)));
    const size_t had = c->c2r_cnt.bytes;
    CHK(ensure(c->c2r_cnt, CNN2_ROUND_CNT_WORDS * sizeof(unsigned int)));
    if (c->c2r_cnt.bytes != had)  // new: zero once, every group of launches leaves it zero
        HIPCHK(hipMemsetAsync(c->c2r_cnt.p, 0, c->c2r_cnt.bytes, c->stream));
    return BK_OK;
}

// the launches of one linear tile space (the begin's set, or a score group) of
// `samples` samples, at most CNN2_ROUND_TILES tiles each; the last one finishes
int launch_space(bk_ctx *c, Cnn2RoundLaunch &a, int64_t space, int64_t samples) {
    for (int64_t lo = 0; lo < space; lo += CNN2_ROUND_TILES) {
        a.tile_lo = (int)lo;
        a.tiles = (int)(space - lo < CNN2_ROUND_TILES ? space - lo : CNN2_ROUND_TILES);
        const int64_t cap = (int64_t)a.tiles * CNN2_TS;
        a.bh = pick_bh(c, a.m, samples < cap ? samples : cap);
        a.finish = a.g > 0 && lo + a.tiles == space;
        const hipError_t he = launch_cnn2_round(a, c->stream);
        if (he != hipSuccess) return fail(BK_EHIP, "k_cnn2_round launch: %s", hipGetErrorString(he));
    }
    return BK_OK;
}

Cnn2RoundLaunch base_launch(bk_ctx *c) {
    Cnn2RoundLaunch a = {};
    a.m = c->c2_dims;
    a.X = (const float *)c->c2_X.p;
    a.y = (const int32_t *)c->c2_y.p;
    a.nv = c->c2_nv;
    a.ww = (const double *)c->c2r_w.p;
    a.flags = (uint8_t *)c->c2r_flags.p;
    a.scratch = (float *)c->c2r_scratch.p;
    a.cnt = (unsigned int *)c->c2r_cnt.p;
    return a;
}

}  // namespace
}  // namespace bk

int bk_roni_cnn2_round_set_band(bk_ctx *c, int rows) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (rows < 0) return fail(BK_EINVAL, "rows=%d < 0", rows);
    std::lock_guard<std::mutex> lk(c->mu);
    c->c2r_band = rows;
    return BK_OK;
}

int bk_roni_cnn2_round_begin(bk_ctx *c, const double *ww, int where) {
    if (!c) return fail(BK_EINVAL, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->c2_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_cnn2_set_validation");
    if (!ww) return fail(BK_EINVAL, "null pointer argument");
    CHK(check_where(where));
    const Cnn2Dims &m = c->c2_dims;
    const int64_t nv = c->c2_nv, space = cnn2_tiles(nv);
    DeviceGuard dg(c->device);
    HostDrain drain{c};
    c->c2r_live = 0;  // no round until the new one's evaluation is queued
    CHK(ensure(c->c2r_w, (size_t)m.d * sizeof(double)));
    CHK(ensure(c->c2r_flags, (size_t)nv));
    CHK(ensure_launch_state(c, space));
    if (!c->ev_round) HIPCHK(hipEventCreateWithFlags(&c->ev_round, hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(c->c2r_w.p, ww, (size_t)m.d * sizeof(double),
                          where == BK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipEventRecord(c->ev_round, c->stream));
    Cnn2RoundLaunch a = base_launch(c);
    CHK(launch_space(c, a, space, nv));  // runs on behind the return
    HIPCHK(hipEventSynchronize(c->ev_round));  // ww is consumed
    drain.armed = false;
    c->c2r_live = 1;
    return BK_OK;
}

int bk_roni_cnn2_round_score_batches(bk_ctx *c, bk_row_table deltas, int64_t count, int where,
                                     const int64_t *idx, int64_t nb, double *scores,
                                     int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!deltas || !idx || !scores) return fail(BK_EINVAL, "null pointer argument");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    if (nb < 1) return fail(BK_EINVAL, "need a batch of nb >= 1 samples (nb=%lld)", (long long)nb);
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->c2_nv < 1) return fail(BK_EINVAL, "no validation set: call bk_roni_cnn2_set_validation");
    if (!c->c2r_live) return fail(BK_EINVAL, "no round: call bk_roni_cnn2_round_begin");
    const Cnn2Dims &m = c->c2_dims;
    const int64_t nv = c->c2_nv, d = m.d;
    if (count > 262139) return fail(BK_ENOTSUP, "RONI n=%lld exceeds 262139", (long long)count);
    if (nb > ((int64_t)1 << 31))
        return fail(BK_ENOTSUP, "the batches' %lld tiles exceed the grid", (long long)cnn2_tiles(nb));
    for (int64_t i = 0; i < count; ++i)
        if (!deltas[i]) return fail(BK_EINVAL, "null row deltas[%lld]", (long long)i);
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
    HostDrain drain{c};  // error returns: queued copies and launches may still read the rows
    const int64_t tpe = cnn2_tiles(nb);
    const int64_t g0 = count < RONI_ROUND_G ? count : RONI_ROUND_G;  // the largest group
    CHK(ensure_launch_state(c, g0 * tpe));
    CHK(ensure_round_out(c, count, 2 * count));
    const double *staged = nullptr;
    if (where != BK_DEVICE) {  // only the rows go up
        CHK(ensure(c->round_rows, (size_t)count * d * sizeof(double)));
        double *dst = (double *)c->round_rows.p;
        for (int64_t i = 0; i < count; ++i)
            HIPCHK(hipMemcpyAsync(dst + i * d, deltas[i], (size_t)d * sizeof(double),
                                  hipMemcpyHostToDevice, c->stream));
        staged = dst;
    }
    // a group's indices ride in its launch's arguments when they fit
    const bool in_args = 2 * g0 * nb <= ROUND_IDX_ARGS;
    if (!in_args) {
        const size_t bytes = (size_t)2 * count * nb * sizeof(int64_t);
        CHK(ensure(c->round_idx, bytes));
        HIPCHK(hipMemcpyAsync(c->round_idx.p, idx, bytes, hipMemcpyHostToDevice, c->stream));
    }
    double *dsc = (double *)c->round_out_dev;
    int32_t *dnt = (int32_t *)(dsc + count);
    for (int64_t q0 = 0; q0 < count; q0 += RONI_ROUND_G) {
        const int g = (int)(count - q0 < RONI_ROUND_G ? count - q0 : RONI_ROUND_G);
        Cnn2RoundLaunch a = base_launch(c);
        a.g = g;
        a.nb = nb;
        for (int q = 0; q < g; ++q) a.rows.p[q] = staged ? staged + (q0 + q) * d : deltas[q0 + q];
        if (in_args)
            for (int64_t i = 0; i < 2 * g * nb; ++i) a.idx_arg.v[i] = (int32_t)idx[2 * q0 * nb + i];
        else
            a.idx_dev = (const int64_t *)c->round_idx.p + 2 * q0 * nb;
        a.scores = dsc + q0;
        a.near = dnt + 2 * q0;
        CHK(launch_space(c, a, g * tpe, g * nb));
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    const char *h = (const char *)c->round_out;
    memcpy(scores, h, (size_t)count * sizeof(double));
    if (near_ties)
        memcpy(near_ties, h + (size_t)count * sizeof(double), (size_t)2 * count * sizeof(int32_t));
    return BK_OK;
}
