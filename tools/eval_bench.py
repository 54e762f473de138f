"""Measure the convergence check (bk_eval, bk_block_finish_eval).

    python tools/eval_bench.py [--out profiles/r24/eval_bench.json] [--parts eval,block]

One process on one GPU; every figure is the median [min .. max] of three runs of
`iters` synchronous calls timed with the host clock, in microseconds per call.

eval   bk_eval of one pageable host model at the creditcard shape (85,000 x 25)
       and at mnist (10,000 x 784, C = 10, plus a 1,000-sample attack set in the
       same call), against
         round_begin  bk_roni_round_begin / bk_roni_softmax_round_begin followed by
                      bk_synchronize on the same set: the nearest same-work call
                      (the same pass over X; the softmax attack set is not in it)
         numpy        sum(sign(X . w) != y) / n, or the argmax of X W^T + b
         torch        the same on torch's CPU tensors
       and, untimed, where bk_eval's time goes: the call from a device model (no
       copy) beside the call from the host model.
block  bk_block_finish_eval against bk_block_finish + bk_eval(BK_HOST) of the
       returned model, with the entry's one-wait route forced (BK_BLOCK_EVAL_SEQ=0)
       and with the sequence inside the entry (BK_BLOCK_EVAL_SEQ=1), at 5 x 25, 35 x 7,850 and 256 x 1,048,576 with a
       matching synthetic set.  The outputs are compared bit for bit first.
Not a pass/fail gate; prints one JSON line per measurement and writes them all.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

RUNS = 3


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def timed(calls, iters):
    """{name: spread of us per call}; the calls alternate within each run."""
    per = {k: [] for k in calls}
    for _ in range(RUNS):
        for name, call in calls.items():
            call()
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            per[name].append((time.perf_counter() - t0) * 1e6 / iters)
    return {k: spread(v) for k, v in per.items()}


def ahead(a, b):
    """a is ahead of b by more than both spreads"""
    return bool(a["max"] < b["min"])


def bench_eval(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    eng = Engine(0)
    rng = np.random.default_rng(20261021)
    out = {"part": "eval", "shape": tag, "runs": RUNS, "device": torch.cuda.get_device_name(0)}
    if tag == "creditcard":
        nv, d, iters = 85000, 25, 200
        X = np.hstack([np.ones((nv, 1)), rng.standard_normal((nv, d - 1))])
        y = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
        ww = rng.standard_normal(d)
        _lib.check(L.bk_roni_set_validation(eng.ctx, X.ctypes.data, nv, d, d, y.ctypes.data))
        eng.eval_set_logistic(0, X, y)
        sets = [0]
        tX, ty, tw = torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(ww)

        def begin():
            _lib.check(L.bk_roni_round_begin(eng.ctx, ww.ctypes.data, d, _lib.BK_HOST))
            eng.synchronize()

        def numpy_ref():
            return np.sum(np.sign(np.dot(X, ww)) != y) / float(y.size)

        def torch_ref():
            return float((torch.sign(tX @ tw) != ty).sum()) / float(nv)
    else:
        nv, din, C, na, iters = 10000, 784, 10, 1000, 50
        d = C * (din + 1)
        X = rng.standard_normal((nv + na, din)).astype(np.float32)
        W = rng.standard_normal((C, din)) * 0.05
        y = np.argmax(X.astype(np.float64) @ W.T, 1).astype(np.int32)
        ww = np.concatenate([W.ravel(), rng.standard_normal(C) * 0.1])
        Xa, ya = X[nv:], y[nv:]
        X, y = X[:nv], y[:nv]
        _lib.check(L.bk_roni_softmax_set_validation(eng.ctx, X.ctypes.data, nv, din, din,
                                                    y.ctypes.data, C))
        eng.eval_set_softmax(1, X, y, C)
        eng.eval_set_softmax(2, Xa, ya, C)
        sets = [1, 2]
        W32, b32 = ww[:C * din].reshape(C, din).astype(np.float32), ww[C * din:].astype(np.float32)
        tX, tXa, tW, tb = (torch.from_numpy(a) for a in (X, Xa, W32, b32))
        ty, tya = torch.from_numpy(y.astype(np.int64)), torch.from_numpy(ya.astype(np.int64))

        def begin():
            _lib.check(L.bk_roni_softmax_round_begin(eng.ctx, ww.ctypes.data, _lib.BK_HOST))
            eng.synchronize()

        def numpy_ref():
            return [1.0 - np.mean(np.argmax(A @ W32.T + b32, axis=1) == l)
                    for A, l in ((X, y), (Xa, ya))]

        def torch_ref():
            return [1.0 - float((torch.argmax(A @ tW.T + tb, dim=1) == l).float().mean())
                    for A, l in ((tX, ty), (tXa, tya))]

    s = np.array(sets, dtype=np.intc)
    err, wrong, near = np.empty(len(sets)), np.empty(len(sets), np.int64), np.empty(len(sets), np.int32)
    dw = torch.from_numpy(ww).cuda()
    torch.cuda.synchronize()

    def host_model():
        eng.eval_ptr(ww.ctypes.data, d, _lib.BK_HOST, s, err, wrong, near)

    def device_model():
        eng.eval_ptr(dw.data_ptr(), d, _lib.BK_DEVICE, s, err, wrong, near)

    host_model()
    out.update(nv=nv, d=d, sets=len(sets), err=err.tolist(), wrong=wrong.tolist(),
               near_ties=near.tolist(), reference_numpy=np.atleast_1d(numpy_ref()).tolist())
    t = timed({"bk_eval": host_model, "round_begin_sync": begin}, iters)
    t.update(timed({"bk_eval_device_model": device_model}, iters))
    t.update(timed({"numpy": numpy_ref, "torch": torch_ref}, max(iters // 10, 3)))
    out["us_per_call"] = t
    out["within_round_begin_spreads"] = not (ahead(t["bk_eval"], t["round_begin_sync"]) or
                                             ahead(t["round_begin_sync"], t["bk_eval"]))
    out["model_copy_us"] = t["bk_eval"]["median"] - t["bk_eval_device_model"]["median"]
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def bench_block(n, d):
    import numpy as np
    import torch
    from biscotti_amd.krum import Engine

    rng = np.random.default_rng(20261022 + n)
    g0 = rng.standard_normal(d)
    rows = [torch.from_numpy(0.01 * rng.standard_normal(d)).pin_memory() for _ in range(min(n, 8))]
    softmax = d == 7850
    if softmax:
        nv = 10000
        X = rng.standard_normal((nv, 784)).astype(np.float32)
        y = rng.integers(0, 10, nv).astype(np.int32)
    else:
        nv = 85000 if d == 25 else 64
        X = rng.standard_normal((nv, d))
        y = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
    iters = 200 if d <= 7850 else 10
    out = {"part": "block", "n": n, "d": d, "set_nv": nv, "runs": RUNS,
           "device": torch.cuda.get_device_name(0)}
    results = {}
    for route in ("one_wait", "sequence"):
        os.environ["BK_BLOCK_EVAL_SEQ"] = "1" if route == "sequence" else "0"  # read by bk_create
        eng = Engine(0)
        if softmax:
            eng.eval_set_softmax(0, X, y, 10)
        else:
            eng.eval_set_logistic(0, X, y)
        eng.block_begin(g0)
        for i in range(n):  # the block's n rows (8 distinct ones)
            tab = (ctypes.c_void_p * 1)(rows[i % len(rows)].data_ptr())
            eng.block_add_ptr(tab, 1, 1)

        def two_calls():
            g = eng.block_finish()
            return (g,) + eng.eval(g, [0])

        def fused():
            return eng.block_finish_eval([0])

        a, b = two_calls(), fused()
        assert all(x.tobytes() == z.tobytes() for x, z in zip(a, b)), "outputs differ"
        t = timed({"finish_then_eval": two_calls, "finish_eval": fused}, iters)
        results[route] = t
        eng.close()
    os.environ.pop("BK_BLOCK_EVAL_SEQ", None)
    out["us_per_call"] = results
    one, seq = results["one_wait"], results["sequence"]
    out["one_wait_ahead_of_two_calls"] = ahead(one["finish_eval"], one["finish_then_eval"])
    out["one_wait_ahead_of_sequence_inside"] = ahead(one["finish_eval"], seq["finish_eval"])
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r24", "eval_bench.json"))
    ap.add_argument("--parts", default="eval,block")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    results = []
    if "eval" in parts:
        results += [bench_eval("creditcard"), bench_eval("mnist")]
    if "block" in parts:
        results += [bench_block(5, 25), bench_block(35, 7850), bench_block(256, 1048576)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/eval_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
