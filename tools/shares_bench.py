#!/usr/bin/env python3
"""Per-call times of the secure-aggregation shares (bk_shares_*).

    python tools/shares_bench.py [--out profiles/r25/shares_bench.json]

One process.  Per shape d (T = 20 shares, 4 miners of 5, 35 clients' parts in the
store, precision 4, host arrays in and out): generate, add (one part), sum over
35 parts and recover, each the median [min..max] of three runs of `--reps`
calls.  generate is timed with both k_shares_gen layouts (one thread per
(chunk, share); one thread per chunk), each in an engine of its own.

BASELINE: a vectorised numpy restatement of each step on the same host.  It is
the only CPU form available here without a Go toolchain -- NOT the reference's
Go code, whose per-share loops (and gonum QR) it does not time.  Parity with Go
is unpinned without Go.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

P, T, MINERS, PREC, PARTS = 10, 20, 4, 4, 35
HELD = T // MINERS
XS = np.arange(T, dtype=np.int64) - 10
I64MIN = np.iinfo(np.int64).min


def np_f2i(a):
    """Go's int64(float64) on an array."""
    ok = (a >= -9223372036854775808.0) & (a < 9223372036854775808.0)
    return np.where(ok, np.where(ok, a, 0.0).astype(np.int64), I64MIN)


def np_generate(delta):
    d = delta.shape[0]
    chunks = -(-d // P)
    c = np.zeros(chunks * P, dtype=np.int64)
    c[:d] = np_f2i(delta * 10.0 ** PREC)
    cf = c.reshape(chunks, P).astype(np.float64)
    xd = XS.astype(np.float64)[None, :]
    y = np.zeros((chunks, T), dtype=np.int64)
    pw = np.ones_like(xd)
    for j in range(P):
        y += np_f2i(pw * cf[:, j:j + 1])
        pw = pw * xd
    c0 = (np_f2i(cf[:, :1]) - y).astype(np.float64)
    h = np.zeros((chunks, T))
    for k in range(P - 1, 0, -1):
        h = cf[:, k:k + 1] - (-xd) * h
    h = c0 - (-xd) * h
    return y + np_f2i(h * 1.0)


def np_recover(w, y):
    """recoverSecret's method, batched: least squares on the Vandermonde matrix."""
    A = np.vander(XS.astype(np.float64), P, increasing=True)
    sol = np.linalg.lstsq(A, y.astype(np.float64).T, rcond=None)[0]
    coef = np.rint(sol).astype(np.int64).T.reshape(-1)[:w.shape[0]]
    return w + coef.astype(np.float64) / 10.0 ** PREC


def timed(fn, reps):
    runs = []
    for _ in range(3):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        runs.append((time.perf_counter() - t0) / reps * 1e6)
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2),
            "max_us": round(max(runs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="25,7850,262144,1048576")
    args = ap.parse_args()
    from biscotti_amd.krum import Engine
    eng = Engine(0)
    os.environ["BK_SHARES_GEN_PER_CHUNK"] = "1"
    eng_pc = Engine(0)
    del os.environ["BK_SHARES_GEN_PER_CHUNK"]
    rows = []
    for d in [int(x) for x in args.shapes.split(",")]:
        rng = np.random.default_rng(d)
        reps = max(3, args.reps // (1 + d // 200000))
        delta = rng.normal(0.0, 0.1, size=d)
        w = rng.normal(size=d)
        chunks = -(-d // P)
        y = eng.shares_generate(delta, PREC, P, T)
        assert np.array_equal(y, eng_pc.shares_generate(delta, PREC, P, T))
        assert np.array_equal(y, np_generate(delta))
        part = np.ascontiguousarray(y[:, :HELD])
        eng.shares_begin(d, P, HELD, PARTS + 1)
        for _ in range(PARTS):
            eng.shares_add(part)
        slots = np.arange(PARTS, dtype=np.int64)
        stack = np.stack([part] * PARTS)

        def add_one():
            # the last slot again and again: begin is not part of the timed call
            eng.shares_begin(d, P, HELD, 1)
            eng.shares_add(part)

        def begin_only():
            eng.shares_begin(d, P, HELD, 1)

        t_add_begin = timed(add_one, reps)
        t_begin = timed(begin_only, reps)
        eng.shares_begin(d, P, HELD, PARTS)
        for _ in range(PARTS):
            eng.shares_add(part)
        agg = eng.shares_sum(slots)
        assert np.array_equal(agg, stack.sum(axis=0))
        parts = [np.ascontiguousarray(y[:, HELD * m:HELD * (m + 1)]) for m in range(MINERS)]
        g, coef, _, bad = eng.shares_recover(w, parts, XS, PREC, P)
        assert bad == 0 and np.array_equal(g, np_recover(w, y))
        row = {
            "d": d, "chunks": chunks, "reps": reps,
            "generate": {"gpu_per_share_thread": timed(lambda: eng.shares_generate(delta, PREC, P, T), reps),
                         "gpu_per_chunk_thread": timed(lambda: eng_pc.shares_generate(delta, PREC, P, T), reps),
                         "numpy": timed(lambda: np_generate(delta), reps)},
            "add": {"gpu_begin_plus_add": t_add_begin, "gpu_begin_alone": t_begin,
                    "numpy": timed(lambda: part.copy(), reps)},
            "sum35": {"gpu": timed(lambda: eng.shares_sum(slots), reps),
                      "numpy": timed(lambda: stack.sum(axis=0), reps)},
            "recover": {"gpu": timed(lambda: eng.shares_recover(w, parts, XS, PREC, P), reps),
                        "numpy_lstsq": timed(lambda: np_recover(w, y), reps)},
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/shares_bench.py", "T": T, "miners": MINERS, "poly_size": P,
           "precision": PREC, "parts_in_store": PARTS,
           "baseline": "vectorised numpy restatement on the same host; not the reference's Go "
                       "code; parity with Go unpinned without Go",
           "shapes": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    eng.close()
    eng_pc.close()


if __name__ == "__main__":
    main()
