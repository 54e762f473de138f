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

    python tools/collect_bench.py --wide [--out profiles/r12/collect_wide_bench.json]

The wide one-launch finish (bk_set_collect_wide) against the same library with
the switch off (the launch chain), at the reference CNN models' shapes -- 100 x
163,850 and 100 x 259,770, fp64 and fp32: per shape the two modes alternate,
three child processes each, and every figure is reported as the median of the
runs' medians with [min .. max] over the runs.  Per run: the finish alone, with
and without a mean (the mean crosses to the host through the mapped block on
the wide path, by a DMA copy on the chain), last add -> finish, the wide
kernel's HIP-event time and its rate over the bytes of the m selected rows,
k_mean's rate in the same run (the packed call's K4 on the same rows), and at
the fp64 shapes the per-problem time of ragged batches of 16 and 64 (n uniform
in 28..100) against the loop of single finishes.
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


WIDE_SHAPES = {"W164_f64": (100, 163850, 30, "float64"), "W260_f64": (100, 259770, 30, "float64"),
               "W164_f32": (100, 163850, 30, "float32"), "W260_f32": (100, 259770, 30, "float32")}
WIDE_REPS, WIDE_RUNS, WIDE_LIMIT = 10, 3, 240


def run_wide(tag, wide):
    """(child) one run of one wide shape with the switch on or off"""
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    n, d, f, dname = WIDE_SHAPES[tag]
    dt = np.dtype(dname)
    es, code = dt.itemsize, (_lib.BK_F64 if dname == "float64" else _lib.BK_F32)
    reps = WIDE_REPS
    L = _lib.lib()
    eng = Engine(0)
    eng.set_collect_wide(wide)
    Xd = torch.empty((n, d), dtype=torch.float64 if es == 8 else torch.float32, device="cuda")
    eng.synth_fill_ptr(Xd.data_ptr(), code, n, d, d, 0, d, 20261019, f)
    eng.synchronize()
    Xp = Xd.cpu().pin_memory()
    m = n - f
    sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
    sc, mean = np.empty(n), np.empty(d)

    def row(i):
        return (ctypes.c_void_p * 1)(Xp.data_ptr() + i * d * es)

    def finish(with_mean=True):
        _lib.check(L.bk_collect_finish(eng.ctx, None, n, f, sel.ctypes.data, ctypes.addressof(mo),
                                       sc.ctypes.data, mean.ctypes.data if with_mean else None))

    def med(call, k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    out = {"shape": tag, "n": n, "d": d, "f": f, "dtype": dname, "reps": reps, "wide": bool(wide),
           "device": torch.cuda.get_device_name(0)}
    # k_mean's rate in this run: the packed call's K4 over the same m x d rows
    def packed():
        _lib.check(L.bk_multikrum(eng.ctx, ctypes.c_void_p(Xp.data_ptr()), _lib.BK_HOST_PINNED, code,
                                  n, d, d, f, sel.ctypes.data, ctypes.addressof(mo),
                                  sc.ctypes.data, mean.ctypes.data))
    packed()
    eng.timing_enable(True)
    for _ in range(3):
        packed()
    tk = eng.timing_read()
    eng.timing_enable(False)
    out["k_mean_ms"] = tk["k_mean"]["avg_ms"]
    out["k_mean_TBps"] = m * d * es / (tk["k_mean"]["avg_ms"] * 1e-3) / 1e12
    packed_sel, packed_mean = sel.copy(), mean.copy()
    last = []
    for _ in range(3):
        eng.collect_begin(n, d, dt)
        for i in range(n - 1):
            eng.collect_add_ptr(row(i), 1, _lib.BK_HOST_PINNED)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.collect_add_ptr(row(n - 1), 1, _lib.BK_HOST_PINNED)
        finish()
        last.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(sel, packed_sel)
        assert np.array_equal(mean.view(np.int64), packed_mean.view(np.int64))
    out["last_add_to_finish_ms"] = statistics.median(last)
    finish()
    out["finish_ms"] = med(finish, 3 * reps)
    out["finish_no_mean_ms"] = med(lambda: finish(False), 3 * reps)
    eng.timing_enable(True)
    for _ in range(reps):
        finish()
    tf = eng.timing_read()
    eng.timing_enable(False)
    eng.timing_enable(True)  # (enabling starts the table afresh)
    for _ in range(reps):
        finish(False)
    tn = eng.timing_read()
    eng.timing_enable(False)
    out["finish_launches"] = {k: v["count"] / reps for k, v in tf.items()}
    out["finish_kernels_avg_ms"] = {k: v["avg_ms"] for k, v in tf.items()}
    out["no_mean_launches"] = {k: v["count"] / reps for k, v in tn.items()}
    if "k_small" in tn:
        out["wide_kernel_no_mean_ms"] = tn["k_small"]["avg_ms"]
    if "k_small" in tf:  # (with a mean the wide launch stops at BK_COLLECT_WIDE_MEAN_MAX_D)
        out["wide_kernel_ms"] = tf["k_small"]["avg_ms"]
        out["wide_kernel_TBps"] = m * d * es / (tf["k_small"]["avg_ms"] * 1e-3) / 1e12
        out["wide_over_k_mean_rate"] = out["wide_kernel_TBps"] / out["k_mean_TBps"]
    if dname == "float64":
        rng = np.random.default_rng(7)
        for B in (16, 64):
            ns = rng.integers(28, 101, size=B)
            orders = [rng.choice(n, size=int(v), replace=False).astype(np.int64) for v in ns]
            fs = [int(v) // 2 for v in ns]
            eng.collect_finish_ragged(orders, fs)

            def loop():
                for o, ff in zip(orders, fs):
                    eng.collect_finish(order=o, f=ff)
            out["ragged%d_per_problem_ms" % B] = med(
                lambda: eng.collect_finish_ragged(orders, fs), 3) / B
            out["loop%d_per_problem_ms" % B] = med(loop, 3) / B
    eng.close()
    print(json.dumps(out), flush=True)


def wide_main(out_path):
    def spread(vals):
        return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}

    results = []
    for tag in sorted(WIDE_SHAPES):
        runs = {"on": [], "off": []}
        for _ in range(WIDE_RUNS):
            for mode in ("on", "off"):  # alternating; a fresh child each, under its own limit
                r = subprocess.run(["timeout", "-k", "10", str(WIDE_LIMIT), sys.executable,
                                    os.path.abspath(__file__), "--wide-shape", tag, "--wide-mode",
                                    mode], stdout=subprocess.PIPE, text=True)
                if r.returncode != 0:
                    print("shape %s (wide %s) failed with status %d" % (tag, mode, r.returncode),
                          file=sys.stderr)
                    return 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                runs[mode].append(json.loads(line))
        rec = dict((k, runs["on"][0][k]) for k in ("shape", "n", "d", "f", "dtype", "device"))
        for mode in ("on", "off"):
            keys = [k for k, v in runs[mode][0].items() if isinstance(v, float)]
            rec["wide_" + mode] = {k: spread([r[k] for r in runs[mode]]) for k in keys}
            rec["wide_" + mode]["finish_launches"] = runs[mode][0]["finish_launches"]
            rec["wide_" + mode]["no_mean_launches"] = runs[mode][0]["no_mean_launches"]
        rec["finish_chain_over_wide"] = (rec["wide_off"]["finish_ms"]["median"] /
                                         rec["wide_on"]["finish_ms"]["median"])
        results.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump({"tool": "tools/collect_bench.py --wide", "runs_per_mode": WIDE_RUNS,
                   "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true",
                    help="the wide one-launch finish against the chain (see the module docstring)")
    ap.add_argument("--wide-shape", choices=sorted(WIDE_SHAPES), help="(child) one wide run")
    ap.add_argument("--wide-mode", choices=("on", "off"), default="on", help="(child)")
    ap.add_argument("--out", help="default: profiles/r08/collect_bench.json, or with --wide "
                                  "profiles/r12/collect_wide_bench.json")
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(child) measure this shape only")
    ap.add_argument("--shapes", default=",".join(sorted(SHAPES)),
                    help="comma-separated shapes to measure (default: all)")
    ap.add_argument("--small-path", choices=("on", "off"), default="on",
                    help="off: n <= 128 calls take the general chain (bk_set_small_path)")
    args = ap.parse_args()
    if args.wide_shape:
        run_wide(args.wide_shape, args.wide_mode == "on")
        return 0
    if args.wide:
        return wide_main(args.out or os.path.join(REPO, "profiles", "r12",
                                                  "collect_wide_bench.json"))
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
    out_path = args.out or os.path.join(REPO, "profiles", "r08", "collect_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump({"tool": "tools/collect_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
