// bk_commit_api.hip -- the host side of bk_commit_* (include/bk.h; the kernels:
// bk_commit.hip; the state: bk_ctx.h struct Commit).
//
// The bn256 G1 commitments of a peer's iteration: createCommitment of the whole
// quantised update (DistSys/honest.go:186, kyber.go:533-562), and
// generateMinerSecretShares' commitments -- the whole update again, every chunk
// of poly_size coefficients and the witness of every (chunk, share)
// (kyber.go:456-482, 172-202, 579-646).  The key PKG1 is resident: set once,
// kept as a table of small multiples.  Every entry is synchronous.  Host inputs
// are copied to a staging buffer of the context, device inputs are read where
// they are; one launch per requested output.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>

#include "bk_ctx.h"

namespace bk {

void commit_destroy(Commit *cm) {
    if (!cm) return;
    if (cm->table) (void)hipFree(cm->table);
    for (DevBuf *b : {&cm->in, &cm->out, &cm->part, &cm->cnt, &cm->bad})
        if (b->p) (void)hipFree(b->p);
    delete cm;
}

}  // namespace bk

namespace {

constexpr size_t POINT = 64;       // a marshalled point
constexpr size_t TABLE_BYTES = 512;  // a key point's table

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

// 10^p, exact for p <= 22 (what Go's math.Pow(10, p) returns)
double scale_of(int precision) {
    double s = 1.0;
    for (int i = 0; i < precision; ++i) s *= 10.0;
    return s;
}

int get_commit(bk_ctx *c, Commit **out) {
    if (!c->commit) {
        c->commit = new (std::nothrow) Commit();
        if (!c->commit) return fail(BK_ENOMEM, "host allocation of the commitment state failed");
        if (const char *v = getenv("BK_COMMIT_MSM_TERMS")) {
            const int t = atoi(v);
            if (t >= 1 && t <= 4096) c->commit->terms = t;
        }
    }
    *out = c->commit;
    return BK_OK;
}

int check_key(const bk_ctx *c, const char *who, int64_t first, int64_t n) {
    if (!c->commit || !c->commit->table) return fail(BK_EINVAL, "%s without bk_commit_set_key", who);
    if (first + n > c->commit->count)
        return fail(BK_EINVAL, "%s: key points [%lld, %lld) past the key's %lld", who,
                    (long long)first, (long long)(first + n), (long long)c->commit->count);
    return BK_OK;
}

// the msm's scratch: the workgroups' sums and the zeroed exit counter
int ensure_msm(bk_ctx *c, Commit *cm) {
    CHK(ensure(cm->part, (size_t)COMMIT_MAX_GROUPS * 24 * 4));
    if (!cm->cnt.p) {
        CHK(ensure(cm->cnt, 4));
        HIPCHK(hipMemsetAsync(cm->cnt.p, 0, 4, c->stream));
    }
    return BK_OK;
}

int check_msm_args(bk_ctx *c, const int64_t *scalars, int where, int64_t n, int64_t key_first) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!scalars) return fail(BK_EINVAL, "null scalars");
    CHK(check_where(where));
    if (n < 1) return fail(BK_EINVAL, "n=%lld < 1", (long long)n);
    if (n > COMMIT_MAX_KEY) return fail(BK_EINVAL, "n=%lld > 2^22", (long long)n);
    if (key_first < 0 || key_first > COMMIT_MAX_KEY)
        return fail(BK_EINVAL, "key_first=%lld outside [0, 2^22]", (long long)key_first);
    return BK_OK;
}

// sum scalars[i] PK[key_first + i] into 64 host bytes or, out_dev, device bytes.
// Under the context mutex with the device selected
int msm_locked(bk_ctx *c, const int64_t *scalars, int where, int64_t n, int64_t key_first,
               uint8_t *out_host, uint8_t *out_dev) {
    Commit *cm = c->commit;
    const hipStream_t st = c->stream;
    const int64_t *dq = scalars;
    if (where != BK_DEVICE) {
        CHK(ensure(cm->in, (size_t)n * 8));
        dq = (const int64_t *)cm->in.p;
    }
    if (!out_dev) {
        CHK(ensure(cm->out, POINT));
        out_dev = (uint8_t *)cm->out.p;
    }
    CHK(ensure_msm(c, cm));
    Drain drain{st};
    ++cm->stats[2];
    if (where != BK_DEVICE) {
        HIPCHK(hipMemcpyAsync(cm->in.p, scalars, (size_t)n * 8, hipMemcpyHostToDevice, st));
        ++cm->stats[1];
    }
    const hipError_t e =
        launch_commit_msm(nullptr, dq, 1.0, n, cm->table + (size_t)key_first * (TABLE_BYTES / 4),
                          (uint32_t *)cm->part.p, (unsigned int *)cm->cnt.p, out_dev, cm->terms, st);
    if (e != hipSuccess) return fail(BK_EHIP, "k_commit_msm launch: %s", hipGetErrorString(e));
    ++cm->stats[0];
    if (out_host) {
        HIPCHK(hipMemcpyAsync(out_host, out_dev, POINT, hipMemcpyDeviceToHost, st));
        ++cm->stats[1];
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    return BK_OK;
}

}  // namespace

int bk_commit_set_key(bk_ctx *c, const uint8_t *pk, int64_t count) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!pk) return fail(BK_EINVAL, "null pk");
    if (count < 1) return fail(BK_EINVAL, "count=%lld < 1", (long long)count);
    if (count > COMMIT_MAX_KEY) return fail(BK_EINVAL, "count=%lld > 2^22", (long long)count);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    Commit *cm = nullptr;
    CHK(get_commit(c, &cm));
    const hipStream_t st = c->stream;
    CHK(ensure(cm->in, (size_t)count * POINT));
    CHK(ensure(cm->bad, 8));
    // the new table beside the resident one, which a refused key leaves in place
    uint32_t *table = nullptr;
    if (hipMalloc(&table, (size_t)count * TABLE_BYTES) != hipSuccess)
        return fail(BK_ENOMEM, "hipMalloc(%zu bytes) of the key table failed",
                    (size_t)count * TABLE_BYTES);
    struct Free {
        uint32_t *p;
        hipStream_t st;
        ~Free() {
            if (!p) return;
            (void)hipStreamSynchronize(st);
            (void)hipFree(p);
        }
    } hold{table, st};
    ++cm->stats[2];
    unsigned long long bad = ~0ull;
    HIPCHK(hipMemcpyAsync(cm->in.p, pk, (size_t)count * POINT, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(cm->bad.p, 0xff, 8, st));
    cm->stats[1] += 1;
    const hipError_t e = launch_commit_key((const uint8_t *)cm->in.p, count, table,
                                           (unsigned long long *)cm->bad.p, st);
    if (e != hipSuccess) return fail(BK_EHIP, "k_commit_key launch: %s", hipGetErrorString(e));
    ++cm->stats[0];
    HIPCHK(hipMemcpyAsync(&bad, cm->bad.p, 8, hipMemcpyDeviceToHost, st));
    ++cm->stats[1];
    HIPCHK(wait_stream(c));
    if (bad != ~0ull)
        return fail(BK_EINVAL, "key point %llu is not a point of G1 (a coordinate >= p or off the curve)",
                    bad);
    if (cm->table) (void)hipFree(cm->table);
    cm->table = table;
    cm->count = count;
    hold.p = nullptr;
    return BK_OK;
}

int bk_commit_key_count(bk_ctx *c, int64_t *count) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!count) return fail(BK_EINVAL, "null count");
    std::lock_guard<std::mutex> lk(c->mu);
    *count = c->commit && c->commit->table ? c->commit->count : 0;
    return BK_OK;
}

int bk_commit_msm(bk_ctx *c, const int64_t *scalars, int where, int64_t n, int64_t key_first,
                  uint8_t *out64) {
    CHK(check_msm_args(c, scalars, where, n, key_first));
    if (!out64) return fail(BK_EINVAL, "null out64");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_key(c, "bk_commit_msm", key_first, n));
    DeviceGuard dg(c->device);
    const bool dev = where == BK_DEVICE;
    return msm_locked(c, scalars, where, n, key_first, dev ? nullptr : out64, dev ? out64 : nullptr);
}

int bk_commit_verify(bk_ctx *c, const int64_t *scalars, int where, int64_t n, int64_t key_first,
                     const uint8_t *committed64, int *ok) {
    CHK(check_msm_args(c, scalars, where, n, key_first));
    if (!committed64) return fail(BK_EINVAL, "null committed64");
    if (!ok) return fail(BK_EINVAL, "null ok");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_key(c, "bk_commit_verify", key_first, n));
    DeviceGuard dg(c->device);
    uint8_t got[POINT], want[POINT];
    if (where == BK_DEVICE) {
        HIPCHK(hipMemcpy(want, committed64, POINT, hipMemcpyDeviceToHost));
        ++c->commit->stats[1];
    } else {
        memcpy(want, committed64, POINT);
    }
    CHK(msm_locked(c, scalars, where, n, key_first, got, nullptr));
    // pointG1.Equal compares the marshalled bytes
    *ok = memcmp(got, want, POINT) == 0 ? 1 : 0;
    return BK_OK;
}

int bk_commit_generate(bk_ctx *c, const double *delta, const int64_t *q, int where, int64_t d,
                       int precision, int poly_size, int total_shares, uint8_t *commit_out,
                       uint8_t *chunk_out, uint8_t *witness_out) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!delta && !q) return fail(BK_EINVAL, "neither delta nor q");
    if (delta && q) return fail(BK_EINVAL, "both delta and q");
    CHK(check_where(where));
    if (d < 1) return fail(BK_EINVAL, "d=%lld < 1", (long long)d);
    if (d > COMMIT_MAX_KEY) return fail(BK_EINVAL, "d=%lld > 2^22", (long long)d);
    if (precision < 0 || precision > 18)
        return fail(BK_ENOTSUP, "precision=%d outside [0, 18]", precision);
    if (poly_size < 1 || poly_size > BK_SHARES_MAX_POLY)
        return fail(BK_ENOTSUP, "poly_size=%d outside [1, %d]", poly_size, BK_SHARES_MAX_POLY);
    if (total_shares < poly_size || total_shares > BK_SHARES_MAX_POINTS)
        return fail(BK_ENOTSUP, "total_shares=%d outside [poly_size=%d, %d]", total_shares,
                    poly_size, BK_SHARES_MAX_POINTS);
    if (!commit_out && !chunk_out && !witness_out) return fail(BK_EINVAL, "no output requested");
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(check_key(c, "bk_commit_generate", 0, d));
    DeviceGuard dg(c->device);
    Commit *cm = c->commit;
    const hipStream_t st = c->stream;
    const bool host = where != BK_DEVICE;
    const int64_t chunks = (d + poly_size - 1) / poly_size;
    const size_t cb = (size_t)chunks * POINT, wb = cb * (size_t)total_shares;
    const double *dd = delta;
    const int64_t *dq = q;
    uint8_t *o_commit = commit_out, *o_chunk = chunk_out, *o_wit = witness_out;
    if (host) {
        CHK(ensure(cm->in, (size_t)d * 8));
        CHK(ensure(cm->out, POINT + cb + wb));
        if (delta) dd = (const double *)cm->in.p;
        else dq = (const int64_t *)cm->in.p;
        o_commit = (uint8_t *)cm->out.p;
        o_chunk = o_commit + POINT;
        o_wit = o_chunk + cb;
    }
    if (commit_out) CHK(ensure_msm(c, cm));
    const double scale = scale_of(precision);
    Drain drain{st};
    ++cm->stats[2];
    if (host) {
        HIPCHK(hipMemcpyAsync(cm->in.p, delta ? (const void *)delta : (const void *)q, (size_t)d * 8,
                              hipMemcpyHostToDevice, st));
        ++cm->stats[1];
    }
    if (commit_out) {
        const hipError_t e = launch_commit_msm(dd, dq, scale, d, cm->table, (uint32_t *)cm->part.p,
                                               (unsigned int *)cm->cnt.p, o_commit, cm->terms, st);
        if (e != hipSuccess) return fail(BK_EHIP, "k_commit_msm launch: %s", hipGetErrorString(e));
        ++cm->stats[0];
    }
    if (chunk_out) {
        const hipError_t e = launch_commit_chunks(dd, dq, scale, d, poly_size, cm->table, o_chunk, st);
        if (e != hipSuccess) return fail(BK_EHIP, "k_commit_chunks launch: %s", hipGetErrorString(e));
        ++cm->stats[0];
    }
    if (witness_out) {
        const hipError_t e = launch_commit_witness(dd, dq, scale, d, poly_size, total_shares,
                                                   cm->table, o_wit, st);
        if (e != hipSuccess) return fail(BK_EHIP, "k_commit_witness launch: %s", hipGetErrorString(e));
        ++cm->stats[0];
    }
    if (host) {
        if (commit_out) {
            HIPCHK(hipMemcpyAsync(commit_out, o_commit, POINT, hipMemcpyDeviceToHost, st));
            ++cm->stats[1];
        }
        if (chunk_out) {
            HIPCHK(hipMemcpyAsync(chunk_out, o_chunk, cb, hipMemcpyDeviceToHost, st));
            ++cm->stats[1];
        }
        if (witness_out) {
            HIPCHK(hipMemcpyAsync(witness_out, o_wit, wb, hipMemcpyDeviceToHost, st));
            ++cm->stats[1];
        }
    }
    HIPCHK(wait_stream(c));
    drain.armed = false;
    return BK_OK;
}

int bk_commit_stats(bk_ctx *c, int64_t out[4]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = 0; i < 3; ++i) out[i] = c->commit ? c->commit->stats[i] : 0;
    out[3] = c->commit && c->commit->table ? c->commit->count : 0;
    return BK_OK;
}
