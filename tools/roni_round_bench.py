"""Measure a RONI round (bk_roni*_round_*) against the loop of one-update calls.

    python tools/roni_round_bench.py [--out profiles/r15/roni_round_bench.json]
                                     [--shapes credit10,credit100,mnist100]

The verifier's iteration as deployed (Peer.VerifyUpdateRONI, main.go:191-233):
n sequential verdicts of ONE update each against one model.  In one process,
per shape and per kind of host rows (pageable, pinned), two ways, alternating:
  loop   n calls of bk_roni / bk_roni_softmax with n = 1 (ww and the update go
         up and the model is evaluated again in every call)
  round  one bk_roni*_round_begin, then n bk_roni*_round_score with count = 1
A run times `iters` such iterations with the host clock (every call is
synchronous) and reports the time per update, the begin included; each figure
is the median [min .. max] of three runs.  The scores of the two ways are
compared bit for bit first.  A further untimed pass reads the launches' HIP-
event times (bk_timing_read).
Shapes: creditcard 85,000 x 25 (n = 10 and 100), mnist 6,000 x 784, C = 10
(n = 100).  Not a pass/fail gate; prints one JSON line per shape and writes
them all.
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

# kind, nv, d (logistic) or d_in (softmax), classes, n, iterations per run
SHAPES = {"credit10": ("logistic", 85000, 25, 0, 10, 40),
          "credit100": ("logistic", 85000, 25, 0, 100, 8),
          "mnist100": ("softmax", 6000, 784, 10, 100, 4)}
RUNS = 3


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def run_shape(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    kind, nv, din, C, n, iters = SHAPES[tag]
    L = _lib.lib()
    eng = Engine(0)
    rng = np.random.default_rng(20261020)
    if kind == "logistic":
        d = din
        X = np.hstack([np.ones((nv, 1)), rng.standard_normal((nv, d - 1))])
        y = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
        ww = rng.standard_normal(d)
        _lib.check(L.bk_roni_set_validation(eng.ctx, X.ctypes.data, nv, d, d, y.ctypes.data))
    else:
        d = C * (din + 1)
        X = rng.standard_normal((nv, din)).astype(np.float32)
        W = rng.standard_normal((C, din)) * 0.05
        y = np.argmax(X.astype(np.float64) @ W.T, 1).astype(np.int32)
        ww = np.concatenate([W.ravel(), rng.standard_normal(C) * 0.1])
        _lib.check(L.bk_roni_softmax_set_validation(eng.ctx, X.ctypes.data, nv, din, din,
                                                    y.ctypes.data, C))
    D = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 0, size=(n, 1))
    out = {"shape": tag, "kind": kind, "nv": nv, "d": d, "n": n, "iters_per_run": iters,
           "runs": RUNS, "device": torch.cuda.get_device_name(0)}
    for rows_kind in ("pageable", "pinned"):
        if rows_kind == "pageable":
            where = _lib.BK_HOST
            wbuf = ww.copy()
            rows = [D[i].copy() for i in range(n)]  # separately allocated
            wp, rp = wbuf.ctypes.data, [r.ctypes.data for r in rows]
        else:
            where = _lib.BK_HOST_PINNED
            wbuf = torch.from_numpy(ww.copy()).pin_memory()
            rows = [torch.from_numpy(D[i].copy()).pin_memory() for i in range(n)]
            wp, rp = wbuf.data_ptr(), [r.data_ptr() for r in rows]
        tabs = [(ctypes.c_void_p * 1)(p) for p in rp]
        s_loop, s_round = np.empty(n), np.empty(n)
        nt = np.empty(2, dtype=np.int32)

        def loop():
            for i in range(n):
                o = s_loop.ctypes.data + 8 * i
                if kind == "logistic":
                    st = L.bk_roni(eng.ctx, wp, rp[i], 1, d, d, o)
                else:
                    st = L.bk_roni_softmax(eng.ctx, wp, rp[i], 1, d, o, nt.ctypes.data)
                _lib.check(st)

        def rnd():
            if kind == "logistic":
                _lib.check(L.bk_roni_round_begin(eng.ctx, wp, d, where))
            else:
                _lib.check(L.bk_roni_softmax_round_begin(eng.ctx, wp, where))
            for i in range(n):
                o = s_round.ctypes.data + 8 * i
                if kind == "logistic":
                    st = L.bk_roni_round_score(eng.ctx, tabs[i], 1, where, o)
                else:
                    st = L.bk_roni_softmax_round_score(eng.ctx, tabs[i], 1, where, o,
                                                       nt.ctypes.data)
                _lib.check(st)

        loop()
        rnd()
        assert np.array_equal(s_loop.view(np.int64), s_round.view(np.int64)), "scores differ"
        per = {"loop": [], "round": []}
        for _ in range(RUNS):
            for name, call in (("loop", loop), ("round", rnd)):  # alternating
                call()
                t0 = time.perf_counter()
                for _ in range(iters):
                    call()
                per[name].append((time.perf_counter() - t0) * 1e6 / (iters * n))
        rec = {"loop_us_per_update": spread(per["loop"]),
               "round_us_per_update": spread(per["round"])}
        rec["loop_over_round"] = (rec["loop_us_per_update"]["median"] /
                                  rec["round_us_per_update"]["median"])
        # the round is ahead by more than the runs' spread when its slowest run
        # beats the loop's fastest
        rec["round_ahead_beyond_spread"] = bool(rec["round_us_per_update"]["max"] <
                                                rec["loop_us_per_update"]["min"])
        # the launches' own times (HIP events; every timed launch adds two records)
        for name, call in (("loop", loop), ("round", rnd)):
            eng.timing_enable(True)
            call()
            tk = eng.timing_read()
            eng.timing_enable(False)
            rec[name + "_launch_avg_us"] = {k: v["avg_ms"] * 1e3 for k, v in tk.items()}
            rec[name + "_launches_per_update"] = {k: v["count"] / n for k, v in tk.items()}
        out[rows_kind] = rec
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15", "roni_round_bench.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES),
                    help="comma-separated shapes to measure (default: all)")
    args = ap.parse_args()
    tags = [t for t in args.shapes.split(",") if t]
    if any(t not in SHAPES for t in tags):
        ap.error("unknown shape in --shapes (have %s)" % ",".join(SHAPES))
    results = [run_shape(t) for t in tags]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/roni_round_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
