// bk_group.hip -- one process, G GPUs (bk_group_*): a context per device, the
// column shards staged and exchanged from one calling thread.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "bk_ctx.h"

struct bk_group {
    std::vector<bk_ctx *> ctx;
    int mode = BK_GROUP_ALLREDUCE;
    std::mutex mu;
    // per-rank device buffers of the call (shard of X, packed Gram, outputs)
    std::vector<DevBuf> X, U, Ug, sel, sc, mean;
    // BK_GROUP_HOST_EXCHANGE: pinned partials [G][usz] and their sum
    void *hpart = nullptr, *hsum = nullptr;
    size_t hbytes = 0;
};

namespace {

// the column shard of rank r out of G (biscotti_amd/dist.py:shard_bounds)
void group_shard(int64_t d, int G, int r, int64_t *c0, int64_t *dl) {
    int64_t per = (d + G - 1) / G;
    per = (per + 7) / 8 * 8;
    const int64_t a = std::min<int64_t>(d, (int64_t)r * per);
    const int64_t b = std::min<int64_t>(d, a + per);
    *c0 = a;
    *dl = b - a;
}

// Error returns of bk_group_multikrum: every device's copy stream may still be
// reading the caller's X, and D2H copies may still be writing sel / scores /
// mean_out, so all streams of all contexts are drained unless disarmed.
struct GroupDrain {
    bk_group *g;
    bool armed = true;
    ~GroupDrain() {
        if (!armed) return;
        for (bk_ctx *c : g->ctx) {
            DeviceGuard dg(c->device);
            if (c->copy) (void)hipStreamSynchronize(c->copy);
            (void)hipStreamSynchronize(c->stream);
        }
    }
};

int group_free_host(bk_group *g) {
    if (g->hpart) (void)hipHostFree(g->hpart);
    if (g->hsum) (void)hipHostFree(g->hsum);
    g->hpart = g->hsum = nullptr;
    g->hbytes = 0;
    return BK_OK;
}

}  // namespace

extern "C" {

int bk_group_create(bk_group **out, int ngpus, const int *devices, int mode) {
    if (!out) return fail(BK_EINVAL, "null out");
    *out = nullptr;
    if (ngpus < 1 || ngpus > 64) return fail(BK_EINVAL, "ngpus=%d out of range", ngpus);
    if (mode < BK_GROUP_ALLREDUCE || mode > BK_GROUP_HOST_EXCHANGE)
        return fail(BK_EINVAL, "bad group mode %d", mode);
    std::vector<int> devs((size_t)ngpus);
    for (int r = 0; r < ngpus; ++r) devs[(size_t)r] = devices ? devices[r] : r;
    if (mode != BK_GROUP_HOST_EXCHANGE)
        for (int a = 0; a < ngpus; ++a)
            for (int b = a + 1; b < ngpus; ++b)
                if (devs[(size_t)a] == devs[(size_t)b])
                    return fail(BK_EINVAL, "RCCL group modes need distinct devices (device %d "
                                           "repeats); use BK_GROUP_HOST_EXCHANGE",
                                devs[(size_t)a]);
    bk_group *g = new (std::nothrow) bk_group();
    if (!g) return fail(BK_ENOMEM, "host allocation of bk_group failed");
    g->mode = mode;
    for (int r = 0; r < ngpus; ++r) {
        bk_ctx *c = nullptr;
        const int st = bk_create(&c, devs[(size_t)r]);
        if (st != BK_OK) {
            bk_group_destroy(g);
            return st;
        }
        g->ctx.push_back(c);
    }
    const size_t G = (size_t)ngpus;
    g->X.resize(G);
    g->U.resize(G);
    g->Ug.resize(G);
    g->sel.resize(G);
    g->sc.resize(G);
    g->mean.resize(G);
    if (mode != BK_GROUP_HOST_EXCHANGE) {
        std::vector<ncclComm_t> comms(G, nullptr);
        const ncclResult_t r = ncclCommInitAll(comms.data(), ngpus, devs.data());
        if (r != ncclSuccess) {
            bk_group_destroy(g);
            return fail(BK_ERCCL, "ncclCommInitAll(%d): %s", ngpus, ncclGetErrorString(r));
        }
        for (int k = 0; k < ngpus; ++k) {  // each context owns (and destroys) its rank
            g->ctx[(size_t)k]->comm = comms[(size_t)k];
            g->ctx[(size_t)k]->nranks = ngpus;
            g->ctx[(size_t)k]->rank = k;
        }
    }
    *out = g;
    return BK_OK;
}

void bk_group_destroy(bk_group *g) {
    if (!g) return;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        bk_ctx *c = g->ctx[r];
        {
            DeviceGuard dg(c->device);
            (void)hipStreamSynchronize(c->stream);
            for (auto *v : {&g->X, &g->U, &g->Ug, &g->sel, &g->sc, &g->mean})
                if (r < v->size() && (*v)[r].p) (void)hipFree((*v)[r].p);
        }
        bk_destroy(c);
    }
    group_free_host(g);
    delete g;
}

int bk_group_size(const bk_group *g) { return g ? (int)g->ctx.size() : 0; }

bk_ctx *bk_group_ctx(bk_group *g, int r) {
    if (!g || r < 0 || r >= (int)g->ctx.size()) return nullptr;
    return g->ctx[(size_t)r];
}

int bk_group_multikrum(bk_group *g, const void *X, int where, int dtype, int64_t n, int64_t d,
                       int64_t ld, int64_t f, int64_t *sel_idx, int64_t *m_out, double *scores,
                       double *mean_out) {
    if (!g || g->ctx.empty()) return fail(BK_EINVAL, "null group");
    CHK(check_common(g->ctx[0], X, dtype, n, d, ld));
    CHK(bk_check_args(n, d, f));
    if (!sel_idx) return fail(BK_EINVAL, "null sel_idx");
    if (where != BK_HOST && where != BK_HOST_PINNED)
        return fail(BK_EINVAL, "bk_group_multikrum takes host X (where=%d)", where);
    const int G = (int)g->ctx.size();
    // Biscotti's deployed shapes (n <= 128, small d: configs A and B) are one
    // launch on one device (k_small); splitting them over devices only adds
    // copies and an exchange
    if (small_ok(g->ctx[0], X, dtype, n, d, ld))
        return bk_multikrum(g->ctx[0], X, where, dtype, n, d, ld, f, sel_idx, m_out, scores,
                            mean_out);
    for (int r = 0; r < G; ++r) {
        int64_t c0, dl;
        group_shard(d, G, r, &c0, &dl);
        if (dl < 1)  // d too small to give every device a column: one device does it all
            return bk_multikrum(g->ctx[0], X, where, dtype, n, d, ld, f, sel_idx, m_out, scores,
                                mean_out);
    }
    std::lock_guard<std::mutex> lk(g->mu);
    std::vector<std::unique_lock<std::mutex>> locks;
    for (bk_ctx *c : g->ctx) locks.emplace_back(c->mu);  // fixed order: no deadlock
    const size_t es = esize(dtype);
    const int64_t m = n - f;
    const int64_t usz = bk_upper_elems(n);
    std::vector<Plan> pls((size_t)G);
    GroupDrain drain{g};
    // 1. per device: its column shard crosses PCIe in column chunks on the
    //    device's copy stream, each chunk's partial Gram (K1 + K1b) overlapped
    //    with the next chunk's copy (stage_host_pipelined)
    for (int r = 0; r < G; ++r) {
        bk_ctx *c = g->ctx[(size_t)r];
        DeviceGuard dg(c->device);
        int64_t c0, dl;
        group_shard(d, G, r, &c0, &dl);
        CHK(ensure(g->X[(size_t)r], (size_t)n * dl * es));
        CHK(ensure(g->U[(size_t)r], (size_t)usz * sizeof(double)));
        const char *src = (const char *)X + (size_t)c0 * es;
        CHK(stage_host_pipelined(c, src, ld, dtype, nullptr, 0, 0, n, dl, (char *)g->X[(size_t)r].p,
                                 dl, (double *)g->U[(size_t)r].p, pls[(size_t)r]));
    }
    // 2.-3. the exchange, then per device the finish and the outputs back
    auto exchange_finish = [&]() -> int {
    if (g->mode == BK_GROUP_ALLREDUCE) {
        RCCLCHK(ncclGroupStart());
        for (int r = 0; r < G; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            double *U = (double *)g->U[(size_t)r].p;
            const ncclResult_t e =
                ncclAllReduce(U, U, (size_t)usz, ncclDouble, ncclSum, c->comm, c->stream);
            if (e != ncclSuccess) {
                (void)ncclGroupEnd();
                return fail(BK_ERCCL, "ncclAllReduce: %s", ncclGetErrorString(e));
            }
        }
        RCCLCHK(ncclGroupEnd());
    } else if (g->mode == BK_GROUP_DETERMINISTIC) {
        for (int r = 0; r < G; ++r) {
            DeviceGuard dg(g->ctx[(size_t)r]->device);
            CHK(ensure(g->Ug[(size_t)r], (size_t)usz * G * sizeof(double)));
        }
        RCCLCHK(ncclGroupStart());
        for (int r = 0; r < G; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            const ncclResult_t e = ncclAllGather(g->U[(size_t)r].p, g->Ug[(size_t)r].p,
                                                 (size_t)usz, ncclDouble, c->comm, c->stream);
            if (e != ncclSuccess) {
                (void)ncclGroupEnd();
                return fail(BK_ERCCL, "ncclAllGather: %s", ncclGetErrorString(e));
            }
        }
        RCCLCHK(ncclGroupEnd());
        for (int r = 0; r < G; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            DeviceGuard dg(c->device);
            HIPCHK(launch_sum_ranks((const double *)g->Ug[(size_t)r].p, G, usz,
                                    (double *)g->U[(size_t)r].p, c->stream));
        }
    } else {  // host exchange: D2H partials, fixed rank-order sum, H2D
        const size_t bytes = (size_t)usz * sizeof(double);
        if (g->hbytes < bytes) {
            group_free_host(g);
            HIPCHK(hipHostMalloc(&g->hpart, bytes * G, hipHostMallocPortable));
            HIPCHK(hipHostMalloc(&g->hsum, bytes, hipHostMallocPortable));
            g->hbytes = bytes;
        }
        double *hp = (double *)g->hpart, *hs = (double *)g->hsum;
        for (int r = 0; r < G; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            DeviceGuard dg(c->device);
            HIPCHK(hipMemcpyAsync(hp + (size_t)r * usz, g->U[(size_t)r].p, bytes,
                                  hipMemcpyDeviceToHost, c->stream));
        }
        for (int r = 0; r < G; ++r) {
            DeviceGuard dg(g->ctx[(size_t)r]->device);
            HIPCHK(hipStreamSynchronize(g->ctx[(size_t)r]->stream));
        }
        for (int64_t e = 0; e < usz; ++e) {  // the order of k_sum_ranks: 0 + U_0 + U_1 + ...
            double acc = 0.0;
            for (int r = 0; r < G; ++r) acc += hp[(size_t)r * usz + e];
            hs[e] = acc;
        }
        for (int r = 0; r < G; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            DeviceGuard dg(c->device);
            HIPCHK(hipMemcpyAsync(g->U[(size_t)r].p, hs, bytes, hipMemcpyHostToDevice, c->stream));
        }
    }
    // 3. per device: scores + selection (identical everywhere), mean of its columns
    for (int r = 0; r < G; ++r) {
        bk_ctx *c = g->ctx[(size_t)r];
        DeviceGuard dg(c->device);
        int64_t c0, dl;
        group_shard(d, G, r, &c0, &dl);
        CHK(ensure(g->sel[(size_t)r], (size_t)n * sizeof(int64_t)));
        CHK(ensure(g->sc[(size_t)r], (size_t)n * sizeof(double)));
        double *dmean = nullptr;
        if (mean_out) {
            CHK(ensure(g->mean[(size_t)r], (size_t)dl * sizeof(double)));
            dmean = (double *)g->mean[(size_t)r].p;
        }
        int64_t *dsel = (int64_t *)g->sel[(size_t)r].p;
        double *dsc = (double *)g->sc[(size_t)r].p;
        CHK(stage_finish(c, (const double *)g->U[(size_t)r].p, pls[(size_t)r], g->X[(size_t)r].p,
                         dtype, n, dl, dl, f, dsel, dsc, dmean));
        CHK(timed(c, BK_K_D2H, [&] {
            hipError_t e = hipSuccess;
            if (r == 0) {
                e = hipMemcpyAsync(sel_idx, dsel, (size_t)m * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess && scores)
                    e = hipMemcpyAsync(scores, dsc, (size_t)n * sizeof(double),
                                       hipMemcpyDeviceToHost, c->stream);
            }
            if (e == hipSuccess && mean_out)
                e = hipMemcpyAsync(mean_out + c0, dmean, (size_t)dl * sizeof(double),
                                   hipMemcpyDeviceToHost, c->stream);
            return e;
        }));
    }
    for (int r = 0; r < G; ++r) {
        DeviceGuard dg(g->ctx[(size_t)r]->device);
        HIPCHK(hipStreamSynchronize(g->ctx[(size_t)r]->stream));
    }
    for (int r = 0; r < G; ++r) CHK(check_margin_readback(g->ctx[(size_t)r]));
    return BK_OK;
    };
    CHK(exchange_finish());
    // BK_F32_CERTIFIED (set on the group's contexts): a near tie of a Gram
    // taken on the fp32 MFMA is re-run exact from the device-resident shards.
    // Every device holds the same summed record, so device 0's margin decides.
    bk_ctx *c0x = g->ctx[0];
    if (certified(c0x, dtype) && c0x->margin_host[2] == 1.0 && c0x->margin_host[8] > 0x1p-53) {
        for (bk_ctx *c : g->ctx) c->force_exact = 1;
        int st = BK_OK;
        for (int r = 0; r < G && st == BK_OK; ++r) {
            bk_ctx *c = g->ctx[(size_t)r];
            DeviceGuard dg(c->device);
            int64_t c0, dl;
            group_shard(d, G, r, &c0, &dl);
            st = stage_gram(c, g->X[(size_t)r].p, dtype, n, dl, dl, (double *)g->U[(size_t)r].p,
                            pls[(size_t)r]);
        }
        if (st == BK_OK) st = exchange_finish();
        for (bk_ctx *c : g->ctx) c->force_exact = 0;
        CHK(st);
        ++c0x->certified_reruns;
    }
    drain.armed = false;
    if (m_out) *m_out = m;
    return BK_OK;
}

}  // extern "C"
