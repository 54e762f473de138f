// bk_block_api.hip -- the host side of bk_block_* (include/bk.h; the kernel:
// bk_block.hip; the state: bk_ctx.h struct Block).
//
// The miner's addBlockUpdate / createBlock (DistSys/honest.go:330-334, :346-388)
// with the add done as each update arrives: a call's rows are cut into launch
// groups of BLOCK_GROUP arrivals, each group one k_block_add that reads the
// running gradient (and quantised sum) once and writes the other copy of it;
// the copies swap when the launch is queued.  The rows of a group come from
// (a) the caller's device memory, (b) a device staging block they are copied to
// (pageable rows through a pinned ring), or (c) a mapped pinned arrival block
// the CPU copies them into and the kernel reads over PCIe -- (c) up to the
// measured row sizes c->block_mapped_* only.  A finish is (x) a D2H copy of the
// current gradient or (y) the stores of a FIN launch into mapped host memory,
// (y) up to c->block_fin_max only.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>

#include "bk_ctx.h"

namespace bk {

void block_destroy(Block *b) {
    if (!b) return;
    for (void *p : {(void *)b->g[0], (void *)b->g[1], (void *)b->q[0], (void *)b->q[1],
                    (void *)b->stage})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)b->ring, (void *)b->arrive, (void *)b->out})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t ev : b->ev_slot)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : b->ev_arrive)
        if (ev) (void)hipEventDestroy(ev);
    if (b->ev_up) (void)hipEventDestroy(b->ev_up);
    delete b;
}

}  // namespace bk

namespace {

// an error path of add / finish: queued copies may still read the caller's rows
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

size_t up16(size_t x) { return (x + 15) / 16 * 16; }

// the bytes of one array of the mapped output block (16-byte aligned starts)
size_t out_stride(int64_t d) { return up16((size_t)d * 8); }

int dev_alloc(void **p, size_t bytes, const char *who) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess)
        return fail(BK_ENOMEM, "%s: hipMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(e));
    return BK_OK;
}

int mapped_alloc(char **hp, char **dp, size_t bytes, unsigned flag, const char *who) {
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocPortable | hipHostMallocMapped | flag);
    if (e != hipSuccess)
        return fail(BK_ENOMEM, "%s: hipHostMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(e));
    e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        return fail(BK_EHIP, "%s: hipHostGetDevicePointer: %s", who, hipGetErrorString(e));
    }
    *hp = (char *)h;
    *dp = (char *)d;
    return BK_OK;
}

// grow-only helpers of add / finish (the block keeps what it has on failure)
int ensure_stage(bk_ctx *c, Block *b, size_t row) {
    const size_t want = row * BLOCK_GROUP;
    if (want <= b->stage_bytes) return BK_OK;
    void *p = nullptr;
    CHK(dev_alloc(&p, want, "bk_block_add"));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b->stage) (void)hipFree(b->stage);
    b->stage = (char *)p;
    b->stage_bytes = want;
    return BK_OK;
}

int ensure_ring(Block *b) {
    if (b->ring) return BK_OK;
    void *p = nullptr;
    const size_t bytes = (size_t)BLOCK_RING_SLOTS * BLOCK_RING_SLOT_BYTES;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e != hipSuccess)
        return fail(BK_ENOMEM, "bk_block_add: hipHostMalloc(%zu bytes): %s", bytes,
                    hipGetErrorString(e));
    for (hipEvent_t &ev : b->ev_slot)
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    b->ring = (char *)p;
    return BK_OK;
}

// the arrival block: BLOCK_ARRIVE_GROUPS launch groups of BLOCK_GROUP rows of
// `row` bytes, coherent on the device's side (every load of a slot crosses PCIe
// and sees what the CPU wrote before the launch)
int ensure_arrive(bk_ctx *c, Block *b, size_t row) {
    if (row <= b->arrive_row) return BK_OK;
    char *hp = nullptr, *dp = nullptr;
    CHK(mapped_alloc(&hp, &dp, row * BLOCK_GROUP * BLOCK_ARRIVE_GROUPS, hipHostMallocCoherent,
                     "bk_block_add"));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b->arrive) (void)hipHostFree(b->arrive);
    for (hipEvent_t &ev : b->ev_arrive)
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (bool &u : b->arrive_used) u = false;
    b->arrive = hp;
    b->arrive_dev = dp;
    b->arrive_row = row;
    return BK_OK;
}

int ensure_out(bk_ctx *c, Block *b) {
    if ((size_t)b->d <= b->out_elems) return BK_OK;
    char *hp = nullptr, *dp = nullptr;
    CHK(mapped_alloc(&hp, &dp, 3 * out_stride(b->d), hipHostMallocNonCoherent, "bk_block"));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b->out) (void)hipHostFree(b->out);
    b->out = hp;
    b->out_dev = dp;
    b->out_elems = (size_t)b->d;
    b->out_valid = false;
    return BK_OK;
}

// one pageable row through the pinned ring: the host copy of a piece overlaps
// the DMA of the one before; on return the row is in the ring or on the device
int upload_pageable(Block *b, char *dst, const char *src, size_t bytes, hipStream_t st) {
    for (size_t off = 0; off < bytes; off += BLOCK_RING_SLOT_BYTES) {
        const size_t len = bytes - off < BLOCK_RING_SLOT_BYTES ? bytes - off : BLOCK_RING_SLOT_BYTES;
        const int s = b->ring_next;
        b->ring_next = (s + 1) % BLOCK_RING_SLOTS;
        if (b->slot_used[s]) HIPCHK(hipEventSynchronize(b->ev_slot[s]));
        char *slot = b->ring + (size_t)s * BLOCK_RING_SLOT_BYTES;
        memcpy(slot, src + off, len);
        HIPCHK(hipMemcpyAsync(dst + off, slot, len, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(b->ev_slot[s], st));
        b->slot_used[s] = true;
    }
    return BK_OK;
}

bool fin_ok(const bk_ctx *c, const Block *b) {
    return (int64_t)b->d * 8 <= c->block_fin_max;
}

// the launch of one group, out of place: reads g / q [cur], writes the other
// pair, which becomes current once the launch is queued
int launch_group(bk_ctx *c, Block *b, const BlockRows &rows, unsigned acc, bool fin) {
    BlockLaunch L = {};
    L.rows = rows;
    L.acc = acc;
    L.dtype = b->dtype;
    L.d = b->d;
    L.gin = b->g[b->cur];
    L.gout = b->g[b->cur ^ 1];
    if (b->precision >= 0) {
        L.qin = b->q[b->cur];
        L.qout = b->q[b->cur ^ 1];
    }
    L.scale = b->scale;
    L.fin = fin ? 1 : 0;
    if (fin) {
        const size_t s = out_stride(b->d);
        L.hg = (double *)b->out_dev;
        L.hq = (int64_t *)(b->out_dev + s);
        L.hqf = (double *)(b->out_dev + 2 * s);
    }
    CHK(timed(c, BK_K_AGGREGATE, [&] { return launch_block_add(L, c->num_cu, c->stream); }));
    b->cur ^= 1;
    b->out_valid = fin;
    return BK_OK;
}

// bk_block_add past its checks (the context mutex held): the rows in launch
// groups of BLOCK_GROUP arrivals; fin: the last group's launch also stores the
// result into the mapped output block (the caller has made sure of the block
// and waits for the stream).  A group counts once its launch is queued
int add_rows(bk_ctx *c, Block *b, const void *const *rows, const uint8_t *accepted, int64_t count,
             int where, bool fin, int64_t *first_slot) {
    const hipStream_t st = c->stream;
    const size_t es = esize(b->dtype), bytes = (size_t)b->d * es, row = up16(bytes);
    const int64_t j0 = b->added;
    const int64_t cut = where == BK_HOST ? c->block_mapped_host : c->block_mapped_pinned;
    const bool mapped = where != BK_DEVICE && (int64_t)bytes <= cut;
    bool any = false;
    for (int64_t i = 0; i < count && !any; ++i) any = !accepted || accepted[i];
    if (any && where != BK_DEVICE) {
        if (mapped) {
            CHK(ensure_arrive(c, b, row));
        } else {
            CHK(ensure_stage(c, b, row));
            if (where == BK_HOST) CHK(ensure_ring(b));
        }
    }
    if (!b->ev_up) HIPCHK(hipEventCreateWithFlags(&b->ev_up, hipEventDisableTiming));
    Drain drain{st};
    bool queued = false;
    for (int64_t g0 = 0; g0 < count; g0 += BLOCK_GROUP) {
        const int gc = (int)(count - g0 < BLOCK_GROUP ? count - g0 : BLOCK_GROUP);
        const bool last = g0 + gc >= count;
        unsigned acc = 0;
        for (int r = 0; r < gc; ++r)
            if (!accepted || accepted[g0 + r]) acc |= 1u << r;
        int nacc = 0;
        BlockRows R = {};
        if (acc) {
            char *base = b->stage;
            int slot = -1;
            if (mapped) {
                slot = b->arrive_next;
                b->arrive_next = (slot + 1) % BLOCK_ARRIVE_GROUPS;
                if (b->arrive_used[slot]) HIPCHK(hipEventSynchronize(b->ev_arrive[slot]));
                base = b->arrive + (size_t)slot * BLOCK_GROUP * b->arrive_row;
            }
            for (int r = 0; r < gc; ++r) {
                if (!(acc >> r & 1)) continue;
                ++nacc;
                const void *src = rows[g0 + r];
                if (where == BK_DEVICE) {
                    R.p[r] = src;
                } else if (mapped) {
                    char *dst = base + (size_t)r * b->arrive_row;
                    memcpy(dst, src, bytes);
                    R.p[r] = b->arrive_dev + (dst - b->arrive);
                } else {
                    char *dst = base + (size_t)r * row;
                    if (where == BK_HOST)
                        CHK(upload_pageable(b, dst, (const char *)src, bytes, st));
                    else
                        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
                    R.p[r] = dst;
                }
            }
            // pinned rows are read by the copies themselves
            if (where == BK_HOST_PINNED && !mapped) HIPCHK(hipEventRecord(b->ev_up, st));
            CHK(launch_group(c, b, R, acc, fin && last));
            queued = true;
            if (mapped) {
                HIPCHK(hipEventRecord(b->ev_arrive[slot], st));
                b->arrive_used[slot] = true;
                ++b->stats[2];
            }
            ++b->stats[fin && last ? 1 : 0];
        } else if (fin && last) {
            // a rejected last arrival: the finish alone rides on the launch
            CHK(launch_group(c, b, R, 0, true));
            ++b->stats[1];
        }
        b->added += gc;
        b->accepted += nacc;
    }
    // consumed on return: device rows are read by the kernels, pinned rows by
    // their copies (a fused call waits for the stream anyway)
    if (queued && !fin) {
        if (where == BK_DEVICE) {
            HIPCHK(hipEventRecord(b->ev_up, st));
            HIPCHK(hipEventSynchronize(b->ev_up));
        } else if (where == BK_HOST_PINNED && !mapped) {
            HIPCHK(hipEventSynchronize(b->ev_up));
        }
    }
    drain.armed = false;
    if (first_slot) *first_slot = j0;
    return BK_OK;
}

struct NoBehind {
    int operator()() const { return BK_OK; }
};

// bk_block_finish past its checks (the context mutex held, the device selected).
// behind: more work for the stream, queued once the finish's own is and before
// the one wait (bk_block_finish_eval's evaluation of g[cur])
template <typename F = NoBehind>
int finish(bk_ctx *c, Block *b, double *global_out, int64_t *qsum_out, double *qsum_float_out,
           F &&behind = F()) {
    const hipStream_t st = c->stream;
    const size_t db = (size_t)b->d * 8, s = out_stride(b->d);
    Drain drain{st};
    // (y) up to the measured cut -- and wherever the quotients q / 10^p are
    // asked for, which exist only as a FIN launch's stores
    if (fin_ok(c, b) || qsum_float_out) {
        CHK(ensure_out(c, b));
        if (!b->out_valid) {
            BlockRows none = {};
            CHK(launch_group(c, b, none, 0, true));
        }
        CHK(behind());
        HIPCHK(wait_stream(c));
        drain.armed = false;
        memcpy(global_out, b->out, db);
        if (qsum_out) memcpy(qsum_out, b->out + s, db);
        if (qsum_float_out) memcpy(qsum_float_out, b->out + 2 * s, db);
        ++b->stats[3];
        return BK_OK;
    }
    CHK(timed(c, BK_K_D2H, [&] {
        hipError_t e = hipMemcpyAsync(global_out, b->g[b->cur], db, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && qsum_out)
            e = hipMemcpyAsync(qsum_out, b->q[b->cur], db, hipMemcpyDeviceToHost, st);
        return e;
    }));
    CHK(behind());
    HIPCHK(wait_stream(c));
    drain.armed = false;
    return BK_OK;
}

int check_live(const bk_ctx *c, const char *who) {
    if (!c->block || !c->block->begun) return fail(BK_EINVAL, "%s without bk_block_begin", who);
    return BK_OK;
}

int check_finish_args(const Block *b, const double *global_out, const int64_t *qsum_out,
                      const double *qsum_float_out) {
    if (!global_out) return fail(BK_EINVAL, "null global_out");
    if (b->precision < 0 && (qsum_out || qsum_float_out))
        return fail(BK_EINVAL, "the block was begun with precision -1: it keeps no quantised sum");
    return BK_OK;
}

int check_add(const Block *b, const void *const *rows, int64_t count) {
    if (b->added + count > BK_MAX_N)
        return fail(BK_EINVAL, "%lld rows after %lld exceed BK_MAX_N=%d", (long long)count,
                    (long long)b->added, BK_MAX_N);
    for (int64_t i = 0; i < count; ++i)
        if (!rows[i]) return fail(BK_EINVAL, "null row rows[%lld]", (long long)i);
    return BK_OK;
}

}  // namespace

int bk_block_begin(bk_ctx *c, int dtype, int64_t d, const double *global_w, int where,
                   int precision) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (dtype != BK_F64 && dtype != BK_F32) return fail(BK_EINVAL, "bad dtype=%d", dtype);
    if (d < 1) return fail(BK_EINVAL, "d=%lld < 1", (long long)d);
    if (!global_w) return fail(BK_EINVAL, "null global_w");
    CHK(check_where(where));
    if (precision < -1 || precision > 18)
        return fail(BK_EINVAL, "precision=%d outside [-1, 18]", precision);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (!c->block) {
        c->block = new (std::nothrow) Block();
        if (!c->block) return fail(BK_ENOMEM, "host allocation of the block failed");
    }
    Block *b = c->block;
    // all or nothing: the new buffers first, the old ones freed once all exist
    const size_t elems = (size_t)(d + 1) / 2 * 2;
    void *ng[2] = {nullptr, nullptr}, *nq[2] = {nullptr, nullptr};
    int st = BK_OK;
    if (elems > b->g_elems)
        for (int i = 0; i < 2 && st == BK_OK; ++i) st = dev_alloc(&ng[i], elems * 8, "bk_block_begin");
    if (precision >= 0 && elems > b->q_elems)
        for (int i = 0; i < 2 && st == BK_OK; ++i) st = dev_alloc(&nq[i], elems * 8, "bk_block_begin");
    if (st != BK_OK) {
        for (void *p : {ng[0], ng[1], nq[0], nq[1]})
            if (p) (void)hipFree(p);
        return st;
    }
    if (ng[0] || nq[0]) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            for (void *p : {ng[0], ng[1], nq[0], nq[1]})
                if (p) (void)hipFree(p);
            return fail(BK_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
        }
    }
    if (ng[0]) {
        for (int i = 0; i < 2; ++i) {
            if (b->g[i]) (void)hipFree(b->g[i]);
            b->g[i] = (double *)ng[i];
        }
        b->g_elems = elems;
    }
    if (nq[0]) {
        for (int i = 0; i < 2; ++i) {
            if (b->q[i]) (void)hipFree(b->q[i]);
            b->q[i] = (int64_t *)nq[i];
        }
        b->q_elems = elems;
    }
    b->begun = false;  // no block until the new gradient is on the device
    Drain drain{c->stream};
    if (!b->ev_up) HIPCHK(hipEventCreateWithFlags(&b->ev_up, hipEventDisableTiming));
    CHK(timed(c, BK_K_H2D, [&] {
        return hipMemcpyAsync(b->g[0], global_w, (size_t)d * 8,
                              where == BK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              c->stream);
    }));
    if (precision >= 0) HIPCHK(hipMemsetAsync(b->q[0], 0, (size_t)d * 8, c->stream));
    // global_w is consumed on return
    HIPCHK(hipEventRecord(b->ev_up, c->stream));
    HIPCHK(hipEventSynchronize(b->ev_up));
    drain.armed = false;
    b->dtype = dtype;
    b->d = d;
    b->precision = precision;
    b->scale = 1.0;  // 10^p, exact for p <= 22 (what Go's math.Pow(10, p) returns)
    for (int i = 0; i < precision; ++i) b->scale *= 10.0;
    b->added = b->accepted = 0;
    for (int64_t &s : b->stats) s = 0;
    b->cur = 0;
    b->out_valid = false;
    b->begun = true;
    return BK_OK;
}

int bk_block_add(bk_ctx *c, const void *const *rows, const uint8_t *accepted, int64_t count,
                 int where, int64_t *first_slot) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!rows) return fail(BK_EINVAL, "null rows");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_add"));
    CHK(check_add(c->block, rows, count));
    DeviceGuard dg(c->device);
    return add_rows(c, c->block, rows, accepted, count, where, false, first_slot);
}

int bk_block_count(bk_ctx *c, int64_t *added, int64_t *accepted) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!added || !accepted) return fail(BK_EINVAL, "null added / accepted");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_count"));
    *added = c->block->added;
    *accepted = c->block->accepted;
    return BK_OK;
}

int bk_block_finish(bk_ctx *c, double *global_out, int64_t *qsum_out, double *qsum_float_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!global_out) return fail(BK_EINVAL, "null global_out");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_finish"));
    CHK(check_finish_args(c->block, global_out, qsum_out, qsum_float_out));
    DeviceGuard dg(c->device);
    return finish(c, c->block, global_out, qsum_out, qsum_float_out);
}

int bk_block_add_finish(bk_ctx *c, const void *row, int accepted, int where, int64_t *first_slot,
                        double *global_out, int64_t *qsum_out, double *qsum_float_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!row) return fail(BK_EINVAL, "null row");
    CHK(check_where(where));
    if (!global_out) return fail(BK_EINVAL, "null global_out");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_add_finish"));
    Block *b = c->block;
    CHK(check_finish_args(b, global_out, qsum_out, qsum_float_out));
    const void *const rows[1] = {row};
    CHK(check_add(b, rows, 1));
    DeviceGuard dg(c->device);
    const uint8_t acc = accepted ? 1 : 0;
    // the one-launch form where a FIN launch's stores serve the finish; past
    // that cut the two calls' work inside this entry
    const bool fused = fin_ok(c, b);
    if (fused) CHK(ensure_out(c, b));
    CHK(add_rows(c, b, rows, &acc, 1, where, fused, first_slot));
    return finish(c, b, global_out, qsum_out, qsum_float_out);
}

// createBlock's gradient and checkConvergence's scores of it in one call: the
// evaluation reads g[cur] where the finish leaves it.  One wait for both, or
// the finish, then the evaluation (c->block_eval_one_wait): the same bits
int bk_block_finish_eval(bk_ctx *c, double *global_out, int64_t *qsum_out, double *qsum_float_out,
                         const int *sets, int nsets, double *err, int64_t *wrong,
                         int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!global_out) return fail(BK_EINVAL, "null global_out");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_finish_eval"));
    Block *b = c->block;
    CHK(check_finish_args(b, global_out, qsum_out, qsum_float_out));
    CHK(eval_check_args(sets, nsets, err, wrong));
    CHK(eval_check_sets(c, b->d, sets, nsets));
    DeviceGuard dg(c->device);
    const auto queue = [&] { return eval_queue(c, b->g[b->cur], sets, nsets); };
    // measured: one wait is ahead where the finish is a D2H
    // copy, and behind where it is a FIN launch's stores into mapped memory
    const bool fin = fin_ok(c, b) || qsum_float_out;
    if (c->block_eval_one_wait == 2 || (c->block_eval_one_wait == 1 && !fin)) {
        CHK(finish(c, b, global_out, qsum_out, qsum_float_out, queue));
    } else {
        CHK(finish(c, b, global_out, qsum_out, qsum_float_out));
        Drain drain{c->stream};
        CHK(queue());
        HIPCHK(wait_stream(c));
        drain.armed = false;
    }
    eval_collect(c, nsets, err, wrong, near_ties);
    return BK_OK;
}

int bk_block_stats(bk_ctx *c, int64_t out[4]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_block_stats"));
    for (int i = 0; i < 4; ++i) out[i] = c->block->stats[i];
    return BK_OK;
}
