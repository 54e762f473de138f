#!/usr/bin/env python
"""The miner's last arrival, measured: from the start of the
last add_update to the new model on the host, in one process on one MI355X.

  paths   for d = 25 .. 262,144 (fp64; pinned and pageable rows), each path of
          bk_block_* against the plain one on the other side of its cut: host
          rows read from the mapped arrival block (c) against copied rows (b),
          and the finish through the mapped output (y) against the D2H copy
          (x), alone and as the fused add-finish.  Two engines of this process
          differ in the BK_BLOCK_* knobs only.  A cut is kept where the
          candidate's slowest of three runs is below the plain path's fastest.
  last    for the miner's NUM_SAMPLES / 2 rows (35 x 7,850, 5 x 25, 256 x
          1,048,576 fp64; pinned and pageable, all accepted):
          (i) bk_block_add_finish, (ii) bk_block_add + bk_block_finish,
          (iii) bk_aggregate(BK_HOST_PINNED) on the packed accepted rows,
          (iv) create_block() as it stands; and the host time of one non-last add.

Every figure is the median [min .. max] of three runs; a run is the median of
its repetitions.  Writes profiles/r20/block_bench.json.

    python tools/block_bench.py [--out profiles/r20/block_bench.json] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.aggregate import create_block  # noqa: E402
from biscotti_amd.krum import Engine, Update  # noqa: E402

H, P = _lib.BK_HOST, _lib.BK_HOST_PINNED
KNOBS = ("BK_BLOCK_MAPPED_HOST", "BK_BLOCK_MAPPED_PINNED", "BK_BLOCK_FIN")


def engine_with(mapped, fin):
    old = {k: os.environ.get(k) for k in KNOBS}
    os.environ.update({KNOBS[0]: str(mapped), KNOBS[1]: str(mapped), KNOBS[2]: str(fin)})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def three(fn, reps):
    """median [min .. max] in microseconds of three runs of `reps` calls of fn,
    fn returning the seconds of its timed part"""
    runs = []
    for _ in range(3):
        runs.append(float(np.median([fn() for _ in range(reps)])) * 1e6)
    return {"median_us": float(np.median(runs)), "min_us": min(runs), "max_us": max(runs),
            "reps": reps}


def make_rows(n, d, where, seed=0):
    rng = np.random.default_rng(seed)
    keep = []
    for _ in range(n):
        r = rng.standard_normal(d)
        keep.append(torch.from_numpy(r).pin_memory() if where == P else r)
    ptrs = [k.data_ptr() if where == P else k.ctypes.data for k in keep]
    return keep, ptrs


def tab(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def reps_for(d, n=1):
    return max(3, min(200, int(4e6 // (d * n))))


def bench_paths(plain, cand, ds):
    out = []
    for d in ds:
        g0 = np.random.default_rng(d).standard_normal(d)
        gout = np.empty(d)
        for where, wname in ((P, "pinned"), (H, "pageable")):
            keep, ptrs = make_rows(2, d, where, d)
            t1 = tab(ptrs[:1])
            rec = {"d": d, "rows": wname}
            for e, ename in ((plain, "plain"), (cand, "candidate")):
                e.block_begin(g0)

                def add():
                    t0 = time.perf_counter()
                    e.block_add_ptr(t1, 1, where)
                    e.synchronize()
                    return time.perf_counter() - t0

                def fin():
                    e.block_add_ptr(t1, 1, where)
                    e.synchronize()
                    t0 = time.perf_counter()
                    e.block_finish_ptr(gout.ctypes.data)
                    return time.perf_counter() - t0

                def fused():
                    t0 = time.perf_counter()
                    e.block_add_finish_ptr(ptrs[1], 1, where, gout.ctypes.data)
                    return time.perf_counter() - t0

                def restart(f):
                    def g():
                        if e.block_count()[0] > 16000:
                            e.block_begin(g0)
                        return f()
                    return g
                for f in (add, fin, fused):
                    restart(f)()  # warm up: buffers, first launches
                r = reps_for(d)
                rec[ename] = {"add_sync": three(restart(add), r), "finish": three(restart(fin), r),
                              "add_finish": three(restart(fused), r)}
            # plain.add_sync is (b), candidate's (c); plain.finish is (x), candidate's (y)
            for k in ("add_sync", "finish", "add_finish"):
                rec["keep_" + k] = rec["candidate"][k]["max_us"] < rec["plain"][k]["min_us"]
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def bench_last(eng, shapes):
    out = []
    for n, d in shapes:
        g0 = np.random.default_rng(n).standard_normal(d)
        gout = np.empty(d)
        r = reps_for(d, n)
        for where, wname in ((P, "pinned"), (H, "pageable")):
            keep, ptrs = make_rows(n, d, where, n + d)
            first, last1 = tab(ptrs[:n - 1]), tab(ptrs[n - 1:])
            rec = {"n": n, "d": d, "rows": wname}

            def prefix():
                eng.block_begin(g0)
                eng.block_add_ptr(first, n - 1, where)
                eng.synchronize()

            def i_fused():
                prefix()
                t0 = time.perf_counter()
                eng.block_add_finish_ptr(ptrs[n - 1], 1, where, gout.ctypes.data)
                return time.perf_counter() - t0

            def ii_two():
                prefix()
                t0 = time.perf_counter()
                eng.block_add_ptr(last1, 1, where)
                eng.block_finish_ptr(gout.ctypes.data)
                return time.perf_counter() - t0

            def one_add():
                eng.block_begin(g0)
                eng.synchronize()
                t0 = time.perf_counter()
                eng.block_add_ptr(last1, 1, where)
                return time.perf_counter() - t0
            for f in (i_fused, ii_two, one_add):
                f()
            rec["i_add_finish"] = three(i_fused, r)
            want = gout.copy()
            rec["ii_add_then_finish"] = three(ii_two, r)
            assert np.array_equal(want.view(np.int64), gout.view(np.int64))
            rec["non_last_add_host"] = three(one_add, r)
            out.append(rec)
            print(json.dumps(rec), flush=True)
            del keep
        # (iii) the batch call on rows already packed in pinned memory, (iv) create_block()
        rng = np.random.default_rng(n + d)
        X = torch.empty((n, d), dtype=torch.float64).pin_memory()
        Xn = X.numpy()
        for i in range(n):
            Xn[i] = rng.standard_normal(d)
        idx = np.arange(n, dtype=np.int64)
        g = g0.copy()

        def iii():
            g[:] = g0
            t0 = time.perf_counter()
            _lib.check(_lib.lib().bk_aggregate(eng.ctx, X.data_ptr(), P, _lib.BK_F64, n, d, d,
                                               idx.ctypes.data, n, g.ctypes.data))
            return time.perf_counter() - t0
        ups = [Update(SourceID=i, Delta=Xn[i], Accepted=True) for i in range(n)]

        def iv():
            t0 = time.perf_counter()
            create_block(g0, ups, {}, engine=eng)
            return time.perf_counter() - t0
        iii()
        iv()
        rec = {"n": n, "d": d, "rows": "packed pinned / Update list",
               "iii_bk_aggregate_pinned": three(iii, r), "iv_create_block": three(iv, r)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del X, Xn, ups
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20", "block_bench.json"))
    ap.add_argument("--quick", action="store_true", help="skip the 256 x 1,048,576 shape")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "abi": _lib.BK_ABI_VERSION,
           "code_object": _lib.code_object_sha16()}
    plain, cand = engine_with(0, 0), engine_with(4 << 20, 1 << 40)
    res["paths"] = bench_paths(plain, cand, [25, 128, 784, 7850, 32768, 262144])
    plain.close()
    cand.close()
    eng = Engine(0)  # the product's cuts
    shapes = [(35, 7850), (5, 25)] + ([] if a.quick else [(256, 1 << 20)])
    res["last"] = bench_last(eng, shapes)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
