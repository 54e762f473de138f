// bk_commit_points_api.hip -- the host side of bk_commit_points_* (include/bk.h;
// the kernels: bk_commit_points.hip; the state: bk_ctx.h struct CommitPoints;
// DESIGN.md §5x).
//
// The G1 half of a miner's secure aggregation (DistSys/main.go:151 SECURE_AGG):
// beside the share values of bk_shares_*, a MinerPart carries the client's
// CommitmentUpdate and every chunk's Commitment and held Witnesses
// (extractMinerSecret, kyber.go:205-242), and the reply to GetMinerPart adds
// them point by point over the agreed node list (getSecretShares
// main.go:2157-2189, aggregateSecret kyber.go:244-287).  Every entry is
// synchronous.  Host inputs and outputs go through staging buffers of the
// state, device ones are read and written where they are; one launch per add
// and per sum.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "bk_ctx.h"

namespace bk {

void commit_points_destroy(CommitPoints *cp) {
    if (!cp) return;
    for (DevBuf *b : {&cp->store, &cp->slots, &cp->in, &cp->out, &cp->bad})
        if (b->p) (void)hipFree(b->p);
    delete cp;
}

}  // namespace bk

namespace {

constexpr size_t POINT = 64;  // a marshalled point, and a stored one

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

int get_points(bk_ctx *c, CommitPoints **out) {
    if (!c->points) {
        c->points = new (std::nothrow) CommitPoints();
        if (!c->points) return fail(BK_ENOMEM, "host allocation of the point store's state failed");
    }
    *out = c->points;
    return BK_OK;
}

int check_live(const bk_ctx *c, const char *who) {
    if (!c->points || !c->points->begun)
        return fail(BK_EINVAL, "%s without bk_commit_points_begin", who);
    return BK_OK;
}

}  // namespace

int bk_commit_points_begin(bk_ctx *c, int64_t chunks, int held, int64_t n_cap) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (chunks < 1) return fail(BK_EINVAL, "chunks=%lld < 1", (long long)chunks);
    if (held < 1 || held > BK_SHARES_MAX_POINTS)
        return fail(BK_EINVAL, "held=%d outside [1, %d]", held, BK_SHARES_MAX_POINTS);
    if (n_cap < 1 || n_cap > COMMIT_POINTS_MAX_N)
        return fail(BK_EINVAL, "n_cap=%lld outside [1, %lld]", (long long)n_cap,
                    (long long)COMMIT_POINTS_MAX_N);
    // no device holds 2^31 chunks' rows: refused before the byte count can wrap
    if (chunks > ((int64_t)1 << 31))
        return fail(BK_ENOMEM, "chunks=%lld: a store of that many points cannot be allocated",
                    (long long)chunks);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CommitPoints *cp = nullptr;
    CHK(get_points(c, &cp));
    const int64_t np = 1 + chunks * (1 + (int64_t)held);
    const size_t bytes = (size_t)np * (size_t)n_cap * POINT;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bytes > cp->store.bytes) {
        // the new store before the old one goes: a refusal leaves the state as it was
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BK_ENOMEM, "hipMalloc(%zu bytes) of the point store failed", bytes);
        }
        if (cp->store.p) (void)hipFree(cp->store.p);
        cp->store.p = p;
        cp->store.bytes = bytes;
    }
    cp->chunks = chunks;
    cp->held = held;
    cp->np = np;
    cp->n_cap = n_cap;
    cp->count = 0;
    cp->begun = true;
    return BK_OK;
}

int bk_commit_points_add(bk_ctx *c, const uint8_t *commit64, const uint8_t *chunk_pts,
                         const uint8_t *witness_pts, int where, int64_t *slot) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!commit64) return fail(BK_EINVAL, "null commit64");
    if (!chunk_pts) return fail(BK_EINVAL, "null chunk_pts");
    if (!witness_pts) return fail(BK_EINVAL, "null witness_pts");
    CHK(check_where(where));
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_commit_points_add"));
    CommitPoints *cp = c->points;
    if (cp->count >= cp->n_cap)
        return fail(BK_EINVAL, "the store holds its n_cap=%lld parts", (long long)cp->n_cap);
    DeviceGuard dg(c->device);
    const hipStream_t st = c->stream;
    const size_t cb = (size_t)cp->chunks * POINT, wb = cb * (size_t)cp->held;
    const uint8_t *d_commit = commit64, *d_chunk = chunk_pts, *d_wit = witness_pts;
    if (where != BK_DEVICE) {
        CHK(ensure(cp->in, POINT + cb + wb));
        d_commit = (const uint8_t *)cp->in.p;
        d_chunk = d_commit + POINT;
        d_wit = d_chunk + cb;
    }
    CHK(ensure(cp->bad, 8));
    Drain drain{st};
    ++cp->stats[2];
    if (where != BK_DEVICE) {
        HIPCHK(hipMemcpyAsync((void *)d_commit, commit64, POINT, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void *)d_chunk, chunk_pts, cb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void *)d_wit, witness_pts, wb, hipMemcpyHostToDevice, st));
        cp->stats[1] += 3;
    }
    HIPCHK(hipMemsetAsync(cp->bad.p, 0xff, 8, st));
    uint32_t *row = (uint32_t *)cp->store.p + (size_t)cp->count * (size_t)cp->np * (POINT / 4);
    const hipError_t e = launch_commit_points_in(d_commit, d_chunk, d_wit, cp->held, cp->np, row,
                                                 (unsigned long long *)cp->bad.p, st);
    if (e != hipSuccess)
        return fail(BK_EHIP, "k_commit_points_in launch: %s", hipGetErrorString(e));
    ++cp->stats[0];
    // the bad word is read before the count moves: a refused part takes no slot
    unsigned long long bad = ~0ull;
    HIPCHK(hipMemcpyAsync(&bad, cp->bad.p, 8, hipMemcpyDeviceToHost, st));
    ++cp->stats[1];
    HIPCHK(wait_stream(c));
    drain.armed = false;
    if (bad != ~0ull)
        return fail(BK_EINVAL,
                    "point %llu of the part is not a point of G1 (a coordinate >= p or off the curve)",
                    bad);
    if (slot) *slot = cp->count;
    ++cp->count;
    return BK_OK;
}

int bk_commit_points_count(bk_ctx *c, int64_t *count) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!count) return fail(BK_EINVAL, "null count");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_commit_points_count"));
    *count = c->points->count;
    return BK_OK;
}

int bk_commit_points_set_lanes(bk_ctx *c, int lanes) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8 && lanes != 16)
        return fail(BK_EINVAL, "lanes=%d outside {0, 1, 2, 4, 8, 16}", lanes);
    std::lock_guard<std::mutex> lk(c->mu);
    CommitPoints *cp = nullptr;
    CHK(get_points(c, &cp));
    cp->lanes = lanes;
    return BK_OK;
}

int bk_commit_points_sum(bk_ctx *c, const int64_t *slots, int64_t count, int where,
                         uint8_t *commit_out, uint8_t *chunk_out, uint8_t *witness_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!slots) return fail(BK_EINVAL, "null slots");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    CHK(check_where(where));
    if (!commit_out && !chunk_out && !witness_out) return fail(BK_EINVAL, "no output requested");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_live(c, "bk_commit_points_sum"));
    CommitPoints *cp = c->points;
    if (count > cp->count)
        return fail(BK_EINVAL, "count=%lld exceeds the %lld parts held", (long long)count,
                    (long long)cp->count);
    std::vector<bool> seen((size_t)cp->count, false);
    for (int64_t i = 0; i < count; ++i) {
        const int64_t s = slots[i];
        if (s < 0 || s >= cp->count)
            return fail(BK_EINVAL, "slots[%lld]=%lld outside [0, %lld)", (long long)i, (long long)s,
                        (long long)cp->count);
        if (seen[(size_t)s]) return fail(BK_EINVAL, "slot %lld listed twice", (long long)s);
        seen[(size_t)s] = true;
    }
    DeviceGuard dg(c->device);
    const hipStream_t st = c->stream;
    const bool host = where != BK_DEVICE;
    const size_t cb = (size_t)cp->chunks * POINT, wb = cb * (size_t)cp->held;
    CHK(ensure(cp->slots, (size_t)count * 8));
    uint8_t *o_commit = commit_out, *o_chunk = chunk_out, *o_wit = witness_out;
    if (host) {
        CHK(ensure(cp->out, POINT + cb + wb));
        uint8_t *base = (uint8_t *)cp->out.p;
        o_commit = commit_out ? base : nullptr;
        o_chunk = chunk_out ? base + POINT : nullptr;
        o_wit = witness_out ? base + POINT + cb : nullptr;
    }
    const int lanes = cp->lanes ? cp->lanes : commit_points_lanes(cp->np, count, c->num_cu);
    Drain drain{st};
    ++cp->stats[2];
    HIPCHK(hipMemcpyAsync(cp->slots.p, slots, (size_t)count * 8, hipMemcpyHostToDevice, st));
    ++cp->stats[1];
    const hipError_t e = launch_commit_points_sum(
        (const uint32_t *)cp->store.p, cp->np, cp->held, (const int64_t *)cp->slots.p, count, lanes,
        o_commit, o_chunk, o_wit, st);
    if (e != hipSuccess)
        return fail(BK_EHIP, "k_commit_points_sum launch: %s", hipGetErrorString(e));
    ++cp->stats[0];
    if (host) {
        if (commit_out) {
            HIPCHK(hipMemcpyAsync(commit_out, o_commit, POINT, hipMemcpyDeviceToHost, st));
            ++cp->stats[1];
        }
        if (chunk_out) {
            HIPCHK(hipMemcpyAsync(chunk_out, o_chunk, cb, hipMemcpyDeviceToHost, st));
            ++cp->stats[1];
        }
        if (witness_out) {
            HIPCHK(hipMemcpyAsync(witness_out, o_wit, wb, hipMemcpyDeviceToHost, st));
            ++cp->stats[1];
        }
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    return BK_OK;
}

int bk_commit_points_stats(bk_ctx *c, int64_t out[4]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    const CommitPoints *cp = c->points;
    for (int i = 0; i < 3; ++i) out[i] = cp ? cp->stats[i] : 0;
    out[3] = cp && cp->begun ? cp->count * cp->np : 0;
    return BK_OK;
}
