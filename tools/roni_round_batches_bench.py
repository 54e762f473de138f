"""Measure the softmax round's mini-batch scoring
(bk_roni_softmax_round_score_batches) against the loop of one-update
bk_roni_softmax_batches calls.

    python tools/roni_round_batches_bench.py [--out profiles/r16/roni_round_batches_bench.json]
                                             [--shapes mnist10,mnist100,lfw10]

The mnist / lfw verifier's iteration as deployed (Peer.VerifyUpdateRONI,
main.go:191-233; client_obj.roni on two last mini-batches of 10): n sequential
verdicts of ONE update each against one model.  In one process, per shape and
per kind of host rows (pageable, pinned), two ways, alternating:
  loop   n calls of bk_roni_softmax_batches with n = 1 (ww, the update and the
         indices go up, one k_roni_batch workgroup, the score comes back by copy)
  round  one bk_roni_softmax_round_begin, then n
         bk_roni_softmax_round_score_batches with count = 1
A run times `iters` such iterations with the host clock (every call is
synchronous) and reports the time per update, the begin included; each figure
is the median [min .. max] of three runs.  The scores and near-tie counts of the
two ways are compared bit for bit first.  A further untimed pass reads the
launches' HIP-event times (bk_timing_read).
LIB=<build> loads another build of libbk.so (the kernel variants of DESIGN §5m
were compared that way); --label names it in the record.
Not a pass/fail gate; prints one JSON line per shape and writes them all.
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

from biscotti_amd import _lib  # noqa: E402

if os.environ.get("LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["LIB"])

# nv, d_in, classes, nb, n, iterations per run
SHAPES = {"mnist10": (6000, 784, 10, 10, 10, 40),
          "mnist100": (6000, 784, 10, 10, 100, 8),
          "lfw10": (400, 8742, 12, 10, 10, 20)}
RUNS = 3


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def run_shape(tag):
    import numpy as np
    import torch
    from biscotti_amd.krum import Engine

    nv, din, C, nb, n, iters = SHAPES[tag]
    L = _lib.lib()
    eng = Engine(0)
    rng = np.random.default_rng(20261020)
    d = C * (din + 1)
    X = rng.standard_normal((nv, din)).astype(np.float32)
    W = rng.standard_normal((C, din)) * 0.05
    y = np.argmax(X.astype(np.float64) @ W.T, 1).astype(np.int32)
    ww = np.concatenate([W.ravel(), rng.standard_normal(C) * 0.1])
    _lib.check(L.bk_roni_softmax_set_validation(eng.ctx, X.ctypes.data, nv, din, din,
                                                y.ctypes.data, C))
    D = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 0, size=(n, 1))
    # each update's two last batches, drawn as the DataLoader draws them
    idx = np.array([[rng.permutation(nv)[nv - nb:], rng.permutation(nv)[nv - nb:]]
                    for _ in range(n)], dtype=np.int64)
    out = {"shape": tag, "nv": nv, "d_in": din, "classes": C, "d": d, "nb": nb, "n": n,
           "iters_per_run": iters, "runs": RUNS, "device": torch.cuda.get_device_name(0)}
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
        ip = [idx[i].ctypes.data for i in range(n)]
        s_loop, s_round = np.empty(n), np.empty(n)
        n_loop, n_round = np.empty((n, 2), dtype=np.int32), np.empty((n, 2), dtype=np.int32)

        def loop():
            for i in range(n):
                _lib.check(L.bk_roni_softmax_batches(eng.ctx, wp, rp[i], 1, d, ip[i], nb,
                                                     s_loop.ctypes.data + 8 * i,
                                                     n_loop.ctypes.data + 8 * i))

        def rnd():
            _lib.check(L.bk_roni_softmax_round_begin(eng.ctx, wp, where))
            for i in range(n):
                _lib.check(L.bk_roni_softmax_round_score_batches(
                    eng.ctx, tabs[i], 1, where, ip[i], nb, s_round.ctypes.data + 8 * i,
                    n_round.ctypes.data + 8 * i))

        loop()
        rnd()
        assert np.array_equal(s_loop.view(np.int64), s_round.view(np.int64)), "scores differ"
        assert np.array_equal(n_loop, n_round), "near-tie counts differ"
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16",
                                                  "roni_round_batches_bench.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES),
                    help="comma-separated shapes to measure (default: all)")
    ap.add_argument("--label", default="", help="names the build / knob setting in the record")
    args = ap.parse_args()
    tags = [t for t in args.shapes.split(",") if t]
    if any(t not in SHAPES for t in tags):
        ap.error("unknown shape in --shapes (have %s)" % ",".join(SHAPES))
    results = [run_shape(t) for t in tags]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = {"tool": "tools/roni_round_batches_bench.py", "results": results}
    if args.label:
        rec["label"] = args.label
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
