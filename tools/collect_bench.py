"""Measure the incremental collection (bk_collect_*) against the packed call.

    python tools/collect_bench.py [--out profiles/r08/collect_bench.json]
                                  [--small-path {on,off}] [--shapes A,B,D]

Per shape (A: 10 x 25, B: 100 x 7,850, D: 512 x 1,048,576; fp64, pinned host
rows), in a child process of its own under a time limit:
  1. last_add_to_finish_ms: every row but the last is collected and the stream
     idle (the verifier waiting for its last peer); then the time from the
     start of the last bk_collect_add to the return of bk_collect_finish --
     against bk_multikrum(BK_HOST_PINNED) on the same rows, the cost of the
     same moment without the collection.
  2. border: bk_collect_add of one device-resident row, timed with HIP events
     on the context stream, as a function of the resident rows; bytes = the
     (j + 1) rows the border reads (the row's own D2D copy is in the time, not
     in the bytes) -- against k_mean's streaming rate in the packed call
     (bk_timing_read; m rows read once).
  3. finish_ms: bk_collect_finish alone (gather, K2, K3, K3b, K4, outputs)
     against the packed call's K1b..K4 from bk_timing_read (at B the packed
     call is ONE launch, k_small, which is reported whole), and the launches
     of one finish per kernel from bk_timing_read (finish_launches).
--small-path off runs every n <= 128 call on the general chain
(bk_set_small_path), the collection's finish included: the A/B of the
one-launch finish.
Not a pass/fail gate; prints one JSON line per shape and writes them all.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = {"A": (10, 25, 2, 20, 120), "B": (100, 7850, 30, 20, 120),
          "D": (512, 1048576, 153, 3, 420)}  # n, d, f, reps, limit s


def run_shape(tag, small_path=True):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    n, d, f, reps, _ = SHAPES[tag]
    L = _lib.lib()
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    eng.set_small_path(small_path)
    Xd = torch.empty((n, d), dtype=torch.float64, device="cuda")
    eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64, n, d, d, 0, d, 20261019, f)
    eng.synchronize()
    Xp = Xd.cpu().pin_memory()
    es = 8
    m = n - f
    sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
    sc, mean = np.empty(n), np.empty(d)

    def packed():
        _lib.check(L.bk_multikrum(eng.ctx, ctypes.c_void_p(Xp.data_ptr()), _lib.BK_HOST_PINNED,
                                  _lib.BK_F64, n, d, d, f, sel.ctypes.data, ctypes.addressof(mo),
                                  sc.ctypes.data, mean.ctypes.data))

    def row(t, i):
        return (ctypes.c_void_p * 1)(t.data_ptr() + i * d * es)

    def finish():
        _lib.check(L.bk_collect_finish(eng.ctx, None, n, f, sel.ctypes.data, ctypes.addressof(mo),
                                       sc.ctypes.data, mean.ctypes.data))

    out = {"shape": tag, "n": n, "d": d, "f": f, "dtype": "float64", "reps": reps,
           "small_path": bool(small_path),
           "device": torch.cuda.get_device_name(0)}
    # ---- the packed call: wall time, then its kernels ----------------------
    packed()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        packed()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["packed_pinned_ms"] = {"median": statistics.median(ts), "min": min(ts)}
    packed_sel = sel.copy()
    packed_mean = mean.copy()
    eng.timing_enable(True)
    for _ in range(reps):
        packed()
    tk = eng.timing_read()
    eng.timing_enable(False)
    out["packed_kernels_avg_ms"] = {k: v["avg_ms"] for k, v in tk.items()}
    tail = [k for k in ("k_reduce", "k_transpose", "k_scores", "k_rank", "k_compact", "k_mean")
            if k in tk]
    out["packed_K1b_to_K4_ms"] = (sum(tk[k]["avg_ms"] for k in tail) if tail else None)
    if "k_mean" in tk:
        out["k_mean_TBps"] = m * d * es / (tk["k_mean"]["avg_ms"] * 1e-3) / 1e12
    # ---- 1 and 3: last add -> finish, and the finish alone ---------------------
    last, fin = [], []
    for _ in range(reps):
        eng.collect_begin(n, d, np.float64)
        for i in range(n - 1):
            eng.collect_add_ptr(row(Xp, i), 1, _lib.BK_HOST_PINNED)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.collect_add_ptr(row(Xp, n - 1), 1, _lib.BK_HOST_PINNED)
        finish()
        last.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(sel, packed_sel)
        assert np.array_equal(mean.view(np.int64), packed_mean.view(np.int64))
        for _ in range(3):
            t0 = time.perf_counter()
            finish()
            fin.append((time.perf_counter() - t0) * 1e3)
    out["last_add_to_finish_ms"] = {"median": statistics.median(last), "min": min(last)}
    out["finish_ms"] = {"median": statistics.median(fin), "min": min(fin)}
    out["last_add_to_finish_over_packed"] = (out["last_add_to_finish_ms"]["median"] /
                                             out["packed_pinned_ms"]["median"])
    out["finish_over_packed"] = out["finish_ms"]["median"] / out["packed_pinned_ms"]["median"]
    # the finish's launches per kernel (the collection of the last repetition)
    eng.timing_enable(True)
    for _ in range(reps):
        finish()
    tf = eng.timing_read()
    eng.timing_enable(False)
    out["finish_launches"] = {k: v["count"] / reps for k, v in tf.items()}
    out["finish_kernels_avg_ms"] = {k: v["avg_ms"] for k, v in tf.items()}
    # ---- 2: the border at count = 1 against the resident rows ------------------
    del Xp
    eng.collect_begin(n, d, np.float64)
    evs = []
    for i in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        eng.collect_add_ptr(row(Xd, i), 1, _lib.BK_DEVICE)
        b.record(stream)
        evs.append((a, b))
    eng.synchronize()
    border = []
    marks = sorted({j for j in (0, 7, 15, 31, 63, 99, 127, 255, 383, 511) if j < n} | {n - 1})
    for j in marks:
        # the median of the adds around j (one add is a few us at B)
        near = [evs[q][0].elapsed_time(evs[q][1]) for q in range(max(0, j - 2), min(n, j + 3))]
        ms = statistics.median(near)
        border.append({"resident": j, "add_ms": ms,
                       "TBps": (j + 1) * d * es / (ms * 1e-3) / 1e12})
    out["border_count1"] = border
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08", "collect_bench.json"))
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(child) measure this shape only")
    ap.add_argument("--shapes", default=",".join(sorted(SHAPES)),
                    help="comma-separated shapes to measure (default: all)")
    ap.add_argument("--small-path", choices=("on", "off"), default="on",
                    help="off: n <= 128 calls take the general chain (bk_set_small_path)")
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape, args.small_path == "on")
        return 0
    tags = [t for t in args.shapes.split(",") if t]
    if any(t not in SHAPES for t in tags):
        ap.error("unknown shape in --shapes (have %s)" % ",".join(sorted(SHAPES)))
    results = []
    for tag in tags:
        # a fresh child per shape, under its own time limit; a failed step ends the run
        r = subprocess.run(["timeout", "-k", "10", str(SHAPES[tag][4]), sys.executable,
                            os.path.abspath(__file__), "--shape", tag, "--small-path",
                            args.small_path], stdout=subprocess.PIPE,
                           text=True)
        if r.returncode != 0:
            print("shape %s failed with status %d" % (tag, r.returncode), file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/collect_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
