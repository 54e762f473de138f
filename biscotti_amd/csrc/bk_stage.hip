// bk_stage.hip -- the stages every Multi-Krum entry is made of (bk_ctx.h): K1's
// plans and the K1i8 layouts (cached per shape), the Gram whole or in pieces
// (K1 + K1b), the finish (K2, K3, K3b, K4 and the margin record), the
// one-launch small path, and the waits and margin checks behind them.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bk_ctx.h"

namespace bk {

static Plan make_plan(int64_t n, int64_t d, int num_cu, size_t in_bytes) {
    Plan pl;
    pl.n = (int)n;
    pl.d = d;
    pl.T = (int)((n + 63) / 64);
    pl.ntile = pl.T * (pl.T + 1) / 2;
    const int64_t W = (int64_t)num_cu * 4;  // one wave per SIMD (K1 runs 1 workgroup per CU)
    const size_t part_cap = in_bytes / 16 > (64u << 20) ? in_bytes / 16 : (64u << 20);
    double best_cost = 1e300;
    int best_S = 1;
    for (int S = 1; S <= 4096; ++S) {
        const int64_t kc = ((d + S - 1) / S + 7) / 8 * 8;
        if (S > 1 && kc < 256) break;
        const int64_t Se = (d + kc - 1) / kc;
        if (Se != S) continue;
        if (S > 1 && (size_t)pl.ntile * S * 32768 > part_cap) break;
        const int64_t tasks = (int64_t)pl.ntile * S;
        const int64_t rounds = (tasks + W - 1) / W;
        const double cost = (double)rounds * (double)(kc + 64);  // +64: per-task fixed cost
        if (cost < best_cost * 0.99) {
            best_cost = cost;
            best_S = S;
        }
    }
    pl.S = best_S;
    pl.kc = ((d + best_S - 1) / best_S + 7) / 8 * 8;
    const int64_t tasks = (int64_t)pl.ntile * pl.S;
    pl.nwg = (int)((tasks + 3) / 4);
    return pl;
}

void free_plan(Plan3 &p) {
    if (p.d_groups) (void)hipFree(p.d_groups);
    if (p.d_wg) (void)hipFree(p.d_wg);
    if (p.d_seg) (void)hipFree(p.d_seg);
    if (p.d_red) (void)hipFree(p.d_red);
    if (p.d_wglist) (void)hipFree(p.d_wglist);
    p.d_groups = nullptr;
    p.d_wg = p.d_red = p.d_wglist = p.d_seg = nullptr;
}

int get_plan3(bk_ctx *c, int64_t n, int64_t d, int bk, Plan3 **out) {
    for (auto &cp : c->plans)
        if (cp.n == n && cp.d == d && cp.bk == bk) {
            *out = &cp.p;
            return BK_OK;
        }
    Plan3Host H = build_plan3((int)n, d, c->num_cu, bk);
    for (int u = 0; u < H.ntile; ++u)
        if (H.red[3 * u + 1] < 0) return fail(BK_EHIP, "internal: K1 plan misses sub-tile %d", u);
    Plan3 p;
    p.n = (int)n;
    p.d = d;
    p.T = H.T;
    p.ntile = H.ntile;
    p.ngroups = (int)H.groups.size();
    p.nwg = (int)H.seg.size() / 2;
    p.nvwg = (int)H.wg.size() / 5;
    p.nfull = H.nfull;
    hipError_t e = hipMalloc(&p.d_groups, H.groups.size() * sizeof(GroupDesc));
    if (e == hipSuccess) e = hipMalloc(&p.d_wg, H.wg.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&p.d_seg, H.seg.size() * sizeof(int));
    if (e == hipSuccess)
        e = hipMemcpy(p.d_seg, H.seg.data(), H.seg.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&p.d_red, H.red.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&p.d_wglist, H.wglist.size() * sizeof(int));
    if (e == hipSuccess)
        e = hipMemcpy(p.d_wglist, H.wglist.data(), H.wglist.size() * sizeof(int),
                      hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(p.d_groups, H.groups.data(), H.groups.size() * sizeof(GroupDesc),
                      hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(p.d_wg, H.wg.data(), H.wg.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(p.d_red, H.red.data(), H.red.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_plan(p);
        return fail(BK_ENOMEM, "K1 plan tables: %s", hipGetErrorString(e));
    }
    if (c->plans.size() >= 8) {
        free_plan(c->plans.front().p);
        free_pieces(c->plans.front().pc);
        c->plans.erase(c->plans.begin());
        ++c->ws_epoch;  // a captured graph may point at the evicted tables
    }
    c->plans.push_back({(int)n, d, bk, p});
    *out = &c->plans.back().p;
    return BK_OK;
}

// K1 v3 reads 16-B granules with global_load_lds: every row start must be
// 16-B aligned (fp64: ld even, fp32: ld a multiple of 4)
static bool use_v3(bk_ctx *c, const void *dX, int dtype, int64_t ld) {
    const int64_t epg = dtype == BK_F64 ? 2 : 4;
    return c->gram_variant == 3 && (ld % epg) == 0 && ((uintptr_t)dX % 16) == 0;
}
int v3_bk(int dtype) { return dtype == BK_F64 ? G3_BK : 2 * G3_BK; }

// fp32 rows on the fp32 MFMA for this call: BK_F32_MFMA, or BK_F32_CERTIFIED
// unless its exact re-run of a near tie is in progress
bool f32_mfma_now(const bk_ctx *c, int dtype) {
    return dtype == BK_F32 && !c->force_exact &&
           (c->f32_mode == BK_F32_MFMA || c->f32_mode == BK_F32_CERTIFIED);
}

// rows on the int8-sliced Gram (K1i8) for this call: fp32 rows under
// BK_F32_I8* / BK_F32_I8X2*, fp64 rows under BK_F64_I8* / BK_F64_I8X2*,
// outside a certified exact re-run; 16-B aligned rows, d >= 64.  Returns the
// digit count (3, or 2 for the X2 modes), 0 when the call runs elsewhere
static int i8_now(const bk_ctx *c, const void *dX, int dtype, int64_t d, int64_t ld) {
    const int mode = dtype == BK_F32 ? c->f32_mode : c->f64_mode;
    const int64_t epg = dtype == BK_F32 ? 4 : 2;
    if (c->force_exact || d < 64 || (ld % epg) != 0 || ((uintptr_t)dX % 16) != 0) return 0;
    if (mode == BK_F32_I8 || mode == BK_F32_I8_CERTIFIED) return 3;
    if (mode == BK_F32_I8X2 || mode == BK_F32_I8X2_CERTIFIED) return 2;
    return 0;
}

// K1i8's layout (ranges, tile order) and its device tables, cached per (n, d)
static int get_i8(bk_ctx *c, int64_t n, int64_t d, int es, int ns, bk_ctx::I8Cached **out) {
    for (auto &e : c->i8)
        if (e.n == n && e.d == d && e.L.es == es && e.L.ns == ns) {
            *out = &e;
            return BK_OK;
        }
    bk_ctx::I8Cached e;
    e.n = n;
    e.d = d;
    e.L = i8_layout((int)n, d, es, c->num_cu, ns);
    const size_t tb = (size_t)(e.L.R + 1) * 8 + e.L.order.size() * sizeof(int);
    std::vector<char> h(tb);
    memcpy(h.data(), e.L.rb.data(), (size_t)(e.L.R + 1) * 8);
    memcpy(h.data() + (size_t)(e.L.R + 1) * 8, e.L.order.data(), e.L.order.size() * sizeof(int));
    hipError_t er = hipMalloc(&e.tables, tb);
    if (er == hipSuccess) er = hipMemcpy(e.tables, h.data(), tb, hipMemcpyHostToDevice);
    if (er != hipSuccess) {
        if (e.tables) (void)hipFree(e.tables);
        return fail(BK_ENOMEM, "K1i8 tables: %s", hipGetErrorString(er));
    }
    if (c->i8.size() >= 4) {
        (void)hipFree(c->i8.front().tables);
        free_pieces(c->i8.front().pc);
        c->i8.erase(c->i8.begin());
        ++c->ws_epoch;  // a captured graph may point at the evicted tables
    }
    c->i8.push_back(e);
    *out = &c->i8.back();
    return BK_OK;
}

// K1i8's layout and workspace for this call, or nullptr when the call does not
// take K1i8 -- or cannot: its range partials take R times the packed upper
// (~34 GB at n = 16,384, d = 1M fp32), and a batch the exact path can still
// take is not refused for them, it runs exact (its record then carries no
// int8 bound)
bk_ctx::I8Cached *i8_prepared(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d,
                              int64_t ld) {
    const int ns = i8_now(c, dX, dtype, d, ld);
    if (!ns) return nullptr;
    // a layout whose workspace could not be allocated goes straight to the
    // exact path on later calls: no repeated multi-GB hipMalloc attempts, no
    // workspace freed (and captured graphs retired) every call
    const std::array<int64_t, 4> sig{n, d, (int64_t)esize(dtype), ns};
    for (const auto &f : c->i8_failed)
        if (f == sig) return nullptr;
    const std::string keep = g_err;
    bk_ctx::I8Cached *e = nullptr;
    int st = c->test_i8_enomem ? BK_ENOMEM : get_i8(c, n, d, (int)esize(dtype), ns, &e);
    if (st == BK_OK) st = ensure(c->i8ws, i8_workspace(e->L));
    if (st == BK_OK) return e;
    (void)hipGetLastError();  // a failed hipMalloc must not surface at the next launch check
    g_err = keep;
    c->i8_failed.push_back(sig);
    return nullptr;
}

// Everything stage_gram allocates (K1's plan tables and split-K slabs), so a
// caller can learn of an allocation failure before it launches anything
int prepare_gram(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld) {
    if (i8_prepared(c, dX, dtype, n, d, ld)) return BK_OK;
    if (use_v3(c, dX, dtype, ld)) {
        Plan3 *p3 = nullptr;
        CHK(get_plan3(c, n, d, v3_bk(dtype), &p3));
        return ensure(c->part, (size_t)p3->nvwg * 16 * 4096 * sizeof(double));
    }
    const Plan pl = make_plan(n, d, c->num_cu, (size_t)n * d * esize(dtype));
    return ensure(c->part, (size_t)pl.ntile * pl.S * 4096 * sizeof(double));
}

// A partial that must still join an exchange after its rank failed: the
// trailing pair becomes NaN, every sum with it is NaN, and every rank's finish
// marks the call invalid (MARGIN_POISONED -> BK_ERCCL from bk_synchronize and
// the margin readers)
int poison_upper(bk_ctx *c, double *U, int64_t n) {
    const int64_t T = (n + 63) / 64;
    HIPCHK(hipMemsetAsync(U + T * (T + 1) / 2 * 4096, 0xFF, BK_UPPER_TRAIL * sizeof(double),
                          c->stream));
    return BK_OK;
}

// K1 + K1b: packed upper-triangle Gram of this call's columns into U (tiles,
// then the trailing pair {column count, columns on the fp32 MFMA}, bk_upper_elems)
int stage_gram(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld,
               double *U, Plan &pl) {
    if (bk_ctx::I8Cached *e = i8_prepared(c, dX, dtype, n, d, ld)) {
        // K1i8: digit slices + bound (k_slice), the int8 GEMM (k_gram), the
        // fixed-order sum of the range partials + the record (k_reduce)
        pl.n = (int)n;
        pl.d = d;
        pl.T = (int)((n + 63) / 64);
        pl.ntile = pl.T * (pl.T + 1) / 2;
        const I8Layout &L = e->L;
        void *ws = c->i8ws.p, *tb = e->tables;
        CHK(timed(c, BK_K_SLICE, [&] {
            return launch_i8_slice(dX, dtype, ld, (int)n, d, L, ws, tb, c->stream);
        }));
        CHK(timed(c, BK_K_GRAM, [&] { return launch_i8_gemm((int)n, L, ws, tb, c->stream); }));
        CHK(timed(c, BK_K_REDUCE, [&] { return launch_i8_reduce(d, L, ws, U, c->stream); }));
        return BK_OK;
    }
    if (use_v3(c, dX, dtype, ld)) {
        Plan3 *p3 = nullptr;
        CHK(get_plan3(c, n, d, v3_bk(dtype), &p3));
        pl.n = (int)n;
        pl.d = d;
        pl.T = p3->T;
        pl.ntile = p3->ntile;
        CHK(ensure(c->part, (size_t)p3->nvwg * 16 * 4096 * sizeof(double)));
        double *part = (double *)c->part.p;
        const Plan3 &P3 = *p3;
        long long *trace = nullptr;
        const char *tfile = probe_env("BK_TRACE_FILE");  // debug: per-workgroup timeline
        if (tfile) {
            CHK(ensure(c->trace, (size_t)P3.nwg * 24 * sizeof(long long)));
            HIPCHK(hipMemsetAsync(c->trace.p, 0, (size_t)P3.nwg * 24 * sizeof(long long), c->stream));
            trace = (long long *)c->trace.p;
        }
        CHK(timed(c, BK_K_GRAM, [&] {
            return launch_gram3(dX, dtype, ld, (int)n, d, P3, part, c->stream, c->gram_mode,
                                trace, f32_mfma_now(c, dtype));
        }));
        if (tfile) {
            std::vector<long long> h((size_t)P3.nwg * 24);
            HIPCHK(hipMemcpyAsync(h.data(), trace, h.size() * sizeof(long long),
                                  hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (FILE *fp = fopen(tfile, "ab")) {
                fwrite(h.data(), sizeof(long long), h.size(), fp);
                fclose(fp);
            }
        }
        CHK(timed(c, BK_K_REDUCE, [&] {
            return launch_reduce3(part, P3, U, c->stream, f32_mfma_now(c, dtype));
        }));
        return BK_OK;
    }
    pl = make_plan(n, d, c->num_cu, (size_t)n * d * esize(dtype));
    CHK(ensure(c->part, (size_t)pl.ntile * pl.S * 4096 * sizeof(double)));
    double *part = (double *)c->part.p;
    CHK(timed(c, BK_K_GRAM,
              [&] { return launch_gram(dX, dtype, ld, (int)n, d, pl, part, c->stream); }));
    CHK(timed(c, BK_K_REDUCE, [&] { return launch_reduce(part, pl, U, c->stream); }));
    return BK_OK;
}

// ---- the Gram in pieces, for an exchange overlapped with it ---------------
// (bk_comm_set_mode 2).  The packed upper is
// cut into k contiguous pieces by rows of sub-tiles; piece p is computed by its
// own launches (the same segments / (tile, range) items as the one launch, so
// every sub-tile is bitwise the same), and its all-reduce starts on the
// communication stream while the next pieces compute.

// the device copy of the pieces' tables
static int upload_pieces(Pieces &pc, const std::vector<std::vector<int>> &tabs, int per_item) {
    size_t tot = 0;
    for (auto &t : tabs) {
        pc.off.push_back(tot);
        pc.nwg.push_back((int)(t.size() / per_item));
        tot += t.size();
    }
    std::vector<int> all;
    all.reserve(tot);
    for (auto &t : tabs) all.insert(all.end(), t.begin(), t.end());
    hipError_t e = hipMalloc(&pc.d, std::max<size_t>(tot, 1) * sizeof(int));
    if (e == hipSuccess && tot)
        e = hipMemcpy(pc.d, all.data(), tot * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_pieces(pc);
        return fail(BK_ENOMEM, "piece tables: %s", hipGetErrorString(e));
    }
    pc.ok = true;
    return BK_OK;
}

// The k-piece split of this call's Gram (built once per plan / layout and k):
// *out = nullptr when the call's Gram has none (K1 v1, a McNaughton plan
// whose workgroups span pieces, too few row blocks); then the caller computes
// the Gram whole and exchanges it after
int gram_pieces(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int k,
                const Pieces **out) {
    *out = nullptr;
    const int64_t usz = bk_upper_elems(n);
    auto finish = [&](Pieces &pc, const std::vector<int> &tile_end) {
        pc.e.assign(1, 0);
        for (size_t p = 0; p < tile_end.size(); ++p)
            pc.e.push_back(p + 1 < tile_end.size() ? (int64_t)tile_end[p] * 4096 : usz);
    };
    if (bk_ctx::I8Cached *e = i8_prepared(c, dX, dtype, n, d, ld)) {
        Pieces &pc = e->pc;
        if (pc.k != k) {
            free_pieces(pc);
            pc.k = k;
            std::vector<int> tile_end;
            std::vector<std::vector<int>> orders;
            if (i8_pieces(e->L, k, tile_end, orders)) {
                CHK(upload_pieces(pc, orders, 2));
                finish(pc, tile_end);
            }
        }
        if (pc.ok) *out = &pc;
        return BK_OK;
    }
    if (!use_v3(c, dX, dtype, ld)) return BK_OK;
    Plan3 *p3 = nullptr;
    const int bk = v3_bk(dtype);
    CHK(get_plan3(c, n, d, bk, &p3));
    for (auto &cp : c->plans)
        if (&cp.p == p3) {
            Pieces &pc = cp.pc;
            if (pc.k != k) {
                free_pieces(pc);
                pc.k = k;
                const Plan3Host H = build_plan3((int)n, d, c->num_cu, bk);
                std::vector<int> tile_end;
                std::vector<std::vector<int>> segs;
                if (plan3_pieces(H, k, tile_end, segs)) {
                    CHK(upload_pieces(pc, segs, 2));
                    finish(pc, tile_end);
                }
            }
            if (pc.ok) *out = &pc;
        }
    return BK_OK;
}

// the context's mapped margin record (allocated once: never moves, so a
// captured graph's pointer to it stays valid)
static int margin_rec(bk_ctx *c) {
    if (c->hmargin) return BK_OK;
    void *p = nullptr, *dp = nullptr;
    HIPCHK(hipHostMalloc(&p, 128, hipHostMallocPortable | hipHostMallocMapped |
                                      hipHostMallocNonCoherent));
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) {
        (void)hipHostFree(p);
        return fail(BK_EHIP, "hipHostGetDevicePointer of the margin record failed");
    }
    memset(p, 0, 128);
    c->hmargin = (double *)p;
    c->dmargin = (double *)dp;
    return BK_OK;
}

// The n <= 128 synchronous entries' output block {margin (HOUT_MPAD doubles),
// sel (n), scores (n), mean (d)}: mapped pinned memory the kernel writes
// itself, grown to `words` doubles (grow-only; every user is synchronous, so
// no launch still writes the old block when it is replaced)
int ensure_hout(bk_ctx *c, size_t words) {
    if (c->hout_bytes >= words * sizeof(double)) return BK_OK;
    // an earlier asynchronous call's record may be unchecked: if it lives
    // in the block about to be freed, read it first (its stream is done
    // once wait_stream returns); a record in the context's own block stays
    if (c->margin_host && c->margin_host == c->hout_host_margin) {
        HIPCHK(wait_stream(c));
        if (c->margin_unchecked) {
            c->margin_unchecked = 0;
            CHK(margin_status(c->margin_host));
        }
        c->margin_host = nullptr;
        c->margin_valid = 0;
    }
    if (c->hout) (void)hipHostFree(c->hout);
    c->hout = nullptr;
    c->hout_bytes = 0;
    c->hout_dev = nullptr;
    c->hout_host_margin = nullptr;
    const size_t bytes = std::max<size_t>(words * sizeof(double), 64 * 1024);
#ifdef BK_HOUT_COHERENT  // ablation: uncached host block (each store crosses PCIe at once)
    const unsigned hflags = hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent;
#else  // GPU-cached, written back at the kernel's end: 156 vs 157 us per call at B
    const unsigned hflags = hipHostMallocPortable | hipHostMallocMapped | hipHostMallocNonCoherent;
#endif
    HIPCHK(hipHostMalloc(&c->hout, bytes, hflags));
    c->hout_bytes = bytes;
    void *dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, c->hout, 0));
    c->hout_dev = (double *)dp;
    c->hout_host_margin = (const double *)c->hout;
    return BK_OK;
}

// k_small's queue lines (zeroed once; every launch leaves them zero)
int ensure_small_queue(bk_ctx *c) {
    if (c->small_ctr.p) return BK_OK;
    CHK(ensure(c->small_ctr, SMALL_CTR_WORDS * sizeof(unsigned)));
    HIPCHK(hipMemsetAsync(c->small_ctr.p, 0, SMALL_CTR_WORDS * sizeof(unsigned), c->stream));
    return BK_OK;
}

// stage_finish's workspace, allocated before a sharded call's exchange so that
// a failure is caught by the ranks' status agreement: with split scoring
// stage_finish holds a collective, which no rank may skip
int prepare_finish(bk_ctx *c, int64_t n, const ScoreSplit &sp, bool own_scores) {
    if (sp.parts > 1) {  // first: a rank that fails below can still join the all-gather
        const int64_t ch = (n + sp.parts - 1) / sp.parts;
        CHK(ensure(c->sgather, ((size_t)(ch + 1) * sp.parts + 3) * sizeof(double)));
    }
    CHK(ensure(c->mask, (size_t)n * sizeof(int)));
    if (own_scores) CHK(ensure(c->scores, (size_t)n * sizeof(double)));
    CHK(ensure(c->diag, (size_t)n * sizeof(double)));
    CHK(ensure(c->bnd, 2 * sizeof(double)));
    CHK(margin_rec(c));
    const int T = (int)((n + 63) / 64);
    if (scores_transposed((int)n))
        CHK(ensure(c->Ut, ((size_t)T * (T + 1) / 2 * 4096 + (size_t)T * 64) * sizeof(double)));
    return BK_OK;
}

// a rank whose finish failed before its share still joins the score
// all-gather with a NaN status, so its peers mark the call invalid instead of
// waiting for it.  The gather buffer exists: it is sized by (n, ranks) alone
// and allocated first, on the call whose signature the ranks agreed on
static void join_failed_share(bk_ctx *c, int64_t n, const ScoreSplit &sp) {
    const int64_t ch = (n + sp.parts - 1) / sp.parts;
    if (c->sgather.bytes < ((size_t)(ch + 1) * sp.parts + 3) * sizeof(double)) return;
    double *sg = (double *)c->sgather.p;
    (void)hipMemsetAsync(sg + (size_t)sp.part * (ch + 1) + ch, 0xFF, sizeof(double), c->stream);
    (void)ncclAllGather(sg + (size_t)sp.part * (ch + 1), sg, (size_t)(ch + 1), ncclDouble, c->comm,
                        c->stream);
}

// K2 + K3 + K4 from a packed upper Gram
int stage_finish(bk_ctx *c, const double *U, const Plan &pl, const void *dX, int dtype,
                 int64_t n, int64_t d, int64_t ld, int64_t f, int64_t *d_sel, double *d_scores,
                 double *d_mean, const ScoreSplit &sp) {
    {
        const int pf = prepare_finish(c, n, sp, d_scores == nullptr);
        if (pf != BK_OK) {
            if (sp.mode == SPLIT_RCCL) {
                const std::string msg = g_err;
                join_failed_share(c, n, sp);
                g_err = msg;
            }
            return pf;
        }
    }
    double *sc = d_scores ? d_scores : (double *)c->scores.p;
    int *mask = (int *)c->mask.p;
    double *diag = (double *)c->diag.p, *bnd = (double *)c->bnd.p;
    const int64_t m = n - f;
    const int64_t k = n - f - 2 > 0 ? n - f - 2 : 0;
    // the packed upper's trailing record {column count, columns on the fp32
    // MFMA, int8 error bound, 0}: the margin's d, unit roundoff and absolute
    // Gram error, totals after an exchange
    const double *dcols = U + (size_t)pl.ntile * 4096;
    const double *Ut = nullptr, *dg = nullptr;
    int st = BK_OK;
    if (scores_transposed((int)n)) {
        // large n: transposed off-diagonal tiles + contiguous diagonal, so K2
        // reads rows in 512-B runs (the packed upper's lower half is strided)
        // (split scoring: each share transposes only what its rows read, below)
        const size_t tiles = (size_t)pl.ntile * 4096;
        double *ut = (double *)c->Ut.p;
        if (sp.parts <= 1)
            st = timed(c, BK_K_EXPAND, [&] { return launch_transpose(U, pl.T, ut, ut + tiles, c->stream); });
        Ut = ut;
        dg = ut + tiles;
    }
    if (sp.parts <= 1) {
        CHK(st);
        CHK(timed(c, BK_K_SCORES,
                  [&] { return launch_scores(U, Ut, dg, pl.T, (int)n, k, sc, diag, c->stream); }));
        CHK(timed(c, BK_K_RANK,
                  [&] { return launch_rank(sc, (int)n, (int)m, mask, bnd, c->stream); }));
    } else {
        const int64_t ch = (n + sp.parts - 1) / sp.parts;
        double *sg = (double *)c->sgather.p;
        // share p: the transposed tiles its rows read (block-columns of rows
        // [r0, r1), and the whole diagonal), then its K2, which writes
        // scores[i] of its rows through sg + p, i.e. at p (ch + 1) + (i - p ch);
        // its status word follows at p (ch + 1) + ch
        auto share = [&](int p, bool ok) {
            const int64_t r0 = (int64_t)p * ch, r1 = r0 + ch < n ? r0 + ch : n;
            int s2 = ok ? BK_OK : BK_EHIP;
            if (s2 == BK_OK) {
                const int b0 = r1 > r0 ? (int)(r0 >> 6) : 1, b1 = r1 > r0 ? (int)((r1 - 1) >> 6) : 0;
                double *ut = const_cast<double *>(Ut);
                s2 = timed(c, BK_K_EXPAND, [&] {
                    return launch_transpose(U, pl.T, ut, const_cast<double *>(dg), c->stream, b0, b1);
                });
            }
            if (s2 == BK_OK && r1 > r0)
                s2 = timed(c, BK_K_SCORES, [&] {
                    return launch_scores(U, Ut, dg, pl.T, (int)n, k, sg + p, diag, c->stream,
                                         (int)r0, (int)(r1 - r0));
                });
            const hipError_t e = hipMemsetAsync(sg + (size_t)p * (ch + 1) + ch, s2 == BK_OK ? 0 : 0xFF,
                                                sizeof(double), c->stream);
            if (s2 == BK_OK && e != hipSuccess)
                s2 = fail(BK_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
            return s2;
        };
        if (sp.mode == SPLIT_RCCL) {
            // every rank joins the all-gather, whatever happened to its share
            // (test knob BK_TEST_SPLIT_FAIL=p: this rank's share fails when p - 1
            // is its rank -- tests/test_gpu_rccl_ranks.py, >= 2 GPUs)
            if (st == BK_OK && c->test_split_fail == sp.part + 1)
                st = fail(BK_EHIP, "test knob BK_TEST_SPLIT_FAIL=%d: this rank's share fails",
                          c->test_split_fail);
            const std::string pre = st == BK_OK ? std::string() : g_err;
            const int s2 = share(sp.part, st == BK_OK);
            if (st == BK_OK) st = s2;
            const std::string msg = st == BK_OK ? std::string() : (pre.empty() ? g_err : pre);
            // (timing is best effort here: nothing may keep a rank from the collective)
            hipEvent_t a = nullptr, b = nullptr;
            bool ton = timing_on(c, BK_K_SCORE_GATHER);
            if (ton) {
                const std::string keep = g_err;
                ton = get_event(c, &a) == BK_OK && get_event(c, &b) == BK_OK &&
                      hipEventRecord(a, c->stream) == hipSuccess;
                if (!ton) {
                    if (a) c->pool.push_back(a);
                    if (b) c->pool.push_back(b);
                    g_err = keep;
                }
            }
            RCCLCHK(ncclAllGather(sg + (size_t)sp.part * (ch + 1), sg, (size_t)(ch + 1), ncclDouble,
                                  c->comm, c->stream));
            if (ton) {
                HIPCHK(hipEventRecord(b, c->stream));
                c->pending.push_back({BK_K_SCORE_GATHER, a, b});
            }
            if (st != BK_OK) {
                g_err = msg;
                return st;
            }
        } else {
            CHK(st);
            // one GPU standing in for the ranks: every share (test), or rank
            // 0's once a mode's first call has scored them all (timing
            // emulation: the other shares' scores are that first call's)
            const bool all = sp.mode == SPLIT_TEST || c->emu_split_n != n;
            for (int p = 0; p < sp.parts; ++p) {
                // (test: a share that "fails" is another rank's failure seen
                // from this one -- its NaN status poisons the record below)
                const bool ok = !(sp.mode == SPLIT_TEST && c->test_split_fail == p + 1);
                if (all || p == 0) {
                    const int s2 = share(p, ok);
                    if (ok) CHK(s2);
                }
            }
            if (sp.mode == SPLIT_EMU) c->emu_split_n = n;
        }
        double *rec = sg + (size_t)(ch + 1) * sp.parts;
        HIPCHK(launch_split_unpack(sg, ch, sp.parts, (int)n, dcols, sc, rec, c->stream));
        dcols = rec;
        CHK(timed(c, BK_K_RANK,
                  [&] { return launch_rank(sc, (int)n, (int)m, mask, bnd, c->stream); }));
        diag = const_cast<double *>(dg);  // K2 wrote only its own rows' diag
    }
    CHK(timed(c, BK_K_COMPACT, [&] {
        return launch_compact(mask, (int)n, d_sel, diag, bnd, dcols, k, c->dmargin, c->stream);
    }));
    c->margin_valid = 1;
    c->margin_host = c->hmargin;
    c->margin_unchecked = 1;
    if (d_mean && d > 0) {
        double *seg = nullptr;
        if (mean_segments((int)m) > 1) {
            CHK(ensure(c->mean_part, (size_t)mean_segments((int)m) * (size_t)d * sizeof(double)));
            seg = (double *)c->mean_part.p;
        }
        CHK(timed(c, BK_K_MEAN, [&] {
            return launch_mean(dX, dtype, ld, d, d_sel, (int)m, d_mean, c->num_cu, c->stream, seg);
        }));
    }
    return BK_OK;
}

// k_small (bk_small.hip) takes the whole call for Biscotti's deployed shapes:
// n <= 128 (one 16x16-block grid per wave set) and d small enough that one
// launch beats the chain
bool small_ok(const bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld) {
    static const int64_t dmax = [] {
        const char *e = getenv("BK_SMALL_MAX_D");  // may only lower the cap
        const int64_t v = e ? atoll(e) : (int64_t)32768;
        return v < 32768 ? v : (int64_t)32768;  // d / 64 chunks: <= 1024 G items (k_small's groups)
    }();
    (void)dX;
    (void)dtype;
    (void)ld;  // unaligned rows take k_small's scalar-load variant
    return c->small_on && n <= 128 && d <= dmax;
}

// margin_out / scores_out: the host entry's mapped output block (the record
// and a second copy of the scores written by the kernel straight to host memory)
// g0 / gn / sm: this launch's share -- the G items of chunks [g0, g0 + gn)
// and, with sm, the S and M items (the pipelined host entry, below); the
// default is the whole call in one launch
int run_small(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int64_t f,
              int64_t *d_sel, double *d_scores, double *d_mean, double *margin_out,
              double *scores_out, int g0, int gn, bool sm) {
    const SmallPlan sp = small_plan((int)n, d, c->num_cu);
    CHK(ensure_small_queue(c));
    // per chunk: the full-square partial Gram (16 nb16)^2 + its diagonal (bk_small.hip)
    const size_t np16 = (size_t)16 * sp.nb16;
    CHK(ensure(c->small_part, (size_t)sp.P * (np16 * np16 + np16) * sizeof(double)));
    CHK(ensure(c->U, (size_t)bk_upper_elems(n) * sizeof(double)));
    CHK(ensure(c->diag, (size_t)n * sizeof(double)));
    CHK(margin_rec(c));
    double *sc = d_scores;
    if (!sc) {
        CHK(ensure(c->scores, (size_t)n * sizeof(double)));
        sc = (double *)c->scores.p;
    }
    long long *trace = nullptr;
    const int items = SMALL_SPLIT_ITEMS * (gn < 0 ? sp.P : gn) + (sm ? sp.nS + (d_mean ? sp.C : 1) : 0);
    const int grid = items < c->num_cu ? items : c->num_cu;  // = launch_small's grid
    const size_t twords = (size_t)items * 8 + (size_t)grid * 2;  // + per workgroup {entry, exit}
    const char *tfile = probe_env("BK_SMALL_TRACE");  // debug: per-item timeline
    if (tfile) {
        CHK(ensure(c->trace, twords * sizeof(long long)));
        HIPCHK(hipMemsetAsync(c->trace.p, 0, twords * sizeof(long long), c->stream));
        trace = (long long *)c->trace.p;
    }
    // (the test knob's count goes to launches that wait: a G-only launch has no hand-off)
    const uint64_t spin = c->small_spin_left == 0 || !sm ? SMALL_SPIN_MAX : c->small_spin_max;
    if (c->small_spin_left > 0 && sm) --c->small_spin_left;
    CHK(timed(c, BK_K_SMALL, [&] {
        return launch_small(dX, dtype, ld, (int)n, d, (int)f, sp, (double *)c->small_part.p,
                            (double *)c->U.p, sc, (double *)c->diag.p, d_sel, d_mean,
                            margin_out ? margin_out : c->dmargin,
                            (unsigned *)c->small_ctr.p, c->num_cu, c->stream, trace, spin,
                            c->small_check_lines, scores_out, g0, gn, sm);
    }));
    if (sm) {
        c->margin_valid = 1;
        c->margin_host = margin_out ? c->hout_host_margin : c->hmargin;
        c->margin_unchecked = 1;
    }
    if (tfile) {
        std::vector<long long> h(twords + 6);
        h[0] = items;
        h[1] = SMALL_SPLIT_ITEMS * (gn < 0 ? sp.P : gn);  // G items
        h[2] = sp.Q;
        h[3] = sm ? sp.nS : 0;
        h[4] = sm ? (d_mean ? sp.C : 1) : 0;
        h[5] = grid;
        HIPCHK(hipMemcpyAsync(h.data() + 6, trace, twords * sizeof(long long),
                              hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (FILE *fp = fopen(tfile, "ab")) {
            fwrite(h.data(), sizeof(long long), h.size(), fp);
            fclose(fp);
        }
    }
    return BK_OK;
}

int run_device(bk_ctx *c, const void *dX, int dtype, int64_t n, int64_t d, int64_t ld, int64_t f,
               int64_t *d_sel, double *d_scores, double *d_mean) {
    if (small_ok(c, dX, dtype, n, d, ld))
        return run_small(c, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
    Plan pl;
    const size_t usz = (size_t)bk_upper_elems(n);
    CHK(ensure(c->U, usz * sizeof(double)));
    double *U = (double *)c->U.p;
    CHK(stage_gram(c, dX, dtype, n, d, ld, U, pl));
    return stage_finish(c, U, pl, dX, dtype, n, d, ld, f, d_sel, d_scores, d_mean);
}

// Wait for the context's stream: poll it for up to spin_us, then block.  A
// blocking wait sleeps the host thread until the GPU's completion interrupt;
// after the GPU has idled that wake-up was 40-75 us of a config-B call
// (tools/idle_probe.py: device-resident call after 200 ms idle 152 -> 77 us,
// host entry 229 -> 186 us, with the whole process set to spin).  Polling
// only inside libbk's own waits keeps that without a process-wide flag, and
// the cap bounds the CPU a long call (config D's 76 ms host entry) burns.
// The final hipStreamSynchronize returns at once on a finished stream.
hipError_t wait_stream(bk_ctx *c) {
    if (c->spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        const auto cap = std::chrono::microseconds(c->spin_us);
        for (;;) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q != hipErrorNotReady) {
                if (q != hipSuccess) return q;
                break;
            }
            if (std::chrono::steady_clock::now() - t0 > cap) break;
        }
    }
    return hipStreamSynchronize(c->stream);
}

// the error codes a finish can leave in margin[2] (bk_internal.h MARGIN_*)
int margin_status(const double *mg) {
    if (mg[2] == MARGIN_HANDOFF_TIMEOUT)
        return fail(BK_EHIP, "k_small: a hand-off wait timed out; the call's outputs are invalid "
                             "(sel entries are -1)");
    if (mg[2] == MARGIN_POISONED)
        return fail(BK_ERCCL, "a rank failed before the Gram exchange and poisoned its partial; "
                              "the call's outputs are invalid");
    if (mg[2] == MARGIN_QUEUE_DIRTY)
        return fail(BK_EHIP, "k_small: a queue word other than word 0 of its line was written "
                             "(BK_SMALL_CHECK_LINES)");
    return BK_OK;
}

// the last finish's margin record (k_compact: gap, err_bound, near_tie, M,
// s_lo, s_hi, d, k, then u_G), synchronously
int read_margin(bk_ctx *c, double (&mg)[MARGIN_WORDS]) {
    if (!c->margin_valid || !c->margin_host)
        return fail(BK_EINVAL, "no Multi-Krum call on this context yet");
    // the record sits in mapped host memory (the context's, or the n <= 128
    // host entry's output block): once the stream is done it is readable
    HIPCHK(wait_stream(c));
    // after a batched call: its records are fetched and one picked (bk_batch.hip)
    if (c->margin_host == c->batch_pick) CHK(batch_fetch(c));
    memcpy(mg, c->margin_host, sizeof mg);
    c->margin_unchecked = 0;
    return margin_status(mg);
}

// Synchronous host entries: once their stream has synchronized, the record's
// error codes are checked (it is already in host memory)
int check_margin_readback(bk_ctx *c) {
    c->margin_unchecked = 0;
    return margin_status(c->margin_host);
}

}  // namespace bk
