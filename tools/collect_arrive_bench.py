"""Measure the fused last arrival (bk_collect_add_finish) against the two-call
sequence (bk_collect_add, then bk_collect_finish) it replaces.

    python tools/collect_arrive_bench.py [--out profiles/r17/collect_arrive_bench.json]

Per shape (B: 100 x 7,850 and A: 10 x 25, fp64), row source (pinned, pageable)
and output set (with and without the mean), in ONE process on one GPU: every
row but the last is collected and the stream idle (the verifier waiting for its
last peer); then the wall clock around the C calls, from the start of the last
arrival to the verdict's return -- the fused call and the two-call sequence on
the same rows, alternating (a pageable row of more than 32 KiB is routed to the
sequence inside the entry: `routed_to_sequence`, both sides then run the same
launches).  collect_stats() must show the path each took, and
the two verdicts must agree bitwise.  Three runs (a child process each, under
its own time limit, behind one more that only warms the machine up and is not
counted); every figure is the median of the runs' medians with
[min .. max] over the runs.  `ahead` says whether the fused median is below the
sequence's by more than both sides' spread.  Not a pass/fail gate; prints one
JSON line per run and writes the summary.
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

SHAPES = {"A": (10, 25, 2), "B": (100, 7850, 30)}  # n, d, f
REPS, RUNS, LIMIT = 30, 3, 240
# the parent commit's tools/collect_bench.py, pinned rows with the mean: last
# add -> finish / the finish alone, microseconds (for context only)
PARENT_US = {"B": {"last_add_to_finish": 61, "finish": 39},
             "A": {"last_add_to_finish": 51, "finish": 25}}


def run_once():
    """(child) every configuration once -> one JSON line"""
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "configs": {}}
    for tag, (n, d, f) in sorted(SHAPES.items()):
        Xd = torch.empty((n, d), dtype=torch.float64, device="cuda")
        eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64, n, d, d, 0, d, 20261019, f)
        eng.synchronize()
        Xh = Xd.cpu()
        Xp = Xh.pin_memory()
        m = n - f
        sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
        sc, mean = np.empty(n), np.empty(d)
        for src, X, where in (("pinned", Xp, _lib.BK_HOST_PINNED), ("pageable", Xh, _lib.BK_HOST)):
            base = X.data_ptr()

            def rows(i, k=1):
                return (ctypes.c_void_p * k)(*[base + (i + q) * d * 8 for q in range(k)])

            def resident():
                eng.collect_begin(n, d, np.float64)
                for i in range(0, n - 1, 8):
                    k = min(8, n - 1 - i)
                    eng.collect_add_ptr(rows(i, k), k, where)
                eng.synchronize()
                return eng.collect_stats()

            # a pageable row of more than 32 KiB: the entry runs the two calls itself
            routed = where == _lib.BK_HOST and d * 8 > 32768
            for with_mean in (True, False):
                mp = mean.ctypes.data if with_mean else None
                last = rows(n - 1)

                def fused():
                    _lib.check(L.bk_collect_add_finish(eng.ctx, last[0], where, None, n, f, None,
                                                       sel.ctypes.data, ctypes.addressof(mo),
                                                       sc.ctypes.data, mp))

                def sequence():
                    _lib.check(L.bk_collect_add(eng.ctx, last, 1, where, None))
                    _lib.check(L.bk_collect_finish(eng.ctx, None, n, f, sel.ctypes.data,
                                                   ctypes.addressof(mo), sc.ctypes.data, mp))

                ts = {"fused": [], "sequence": []}
                got = {}
                for r in range(REPS + 3):  # the first three of each: warm-up
                    for name, call in (("fused", fused), ("sequence", sequence)):
                        s0 = resident()
                        t0 = time.perf_counter()
                        call()
                        t1 = time.perf_counter()
                        s1 = eng.collect_stats()
                        took = {k: s1[k] - s0[k] for k in s1}
                        want = ({"border": 0, "border_reduce": 0, "one_launch_finishes": 0,
                                 "fused_arrivals": 1} if name == "fused" and not routed else
                                {"border": 1, "border_reduce": 1, "one_launch_finishes": 1,
                                 "fused_arrivals": 0})
                        assert took == want, (name, took)
                        got[name] = (sel.copy(), sc.copy(), mean.copy() if with_mean else None)
                        if r >= 3:
                            ts[name].append((t1 - t0) * 1e6)
                    assert np.array_equal(got["fused"][0], got["sequence"][0])
                    assert np.array_equal(got["fused"][1].view(np.int64),
                                          got["sequence"][1].view(np.int64))
                    if with_mean:
                        assert np.array_equal(got["fused"][2].view(np.int64),
                                              got["sequence"][2].view(np.int64))
                key = "%s/%s/%s" % (tag, src, "mean" if with_mean else "no_mean")
                out["configs"][key] = {name: {"median_us": statistics.median(v), "min_us": min(v)}
                                       for name, v in ts.items()}
                out["configs"][key]["routed_to_sequence"] = bool(routed)
        del Xp
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(child) one run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17",
                                                  "collect_arrive_bench.json"))
    args = ap.parse_args()
    if args.child:
        run_once()
        return 0
    runs = []
    for k in range(RUNS + 1):  # the first child warms the machine up: printed, not counted
        # a fresh child per run, under its own time limit; a failed run ends the tool
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable,
                            os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("run failed with status %d" % r.returncode, file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if k > 0:
            runs.append(json.loads(line))
    results = {}
    for key in runs[0]["configs"]:
        rec = {}
        for name in ("fused", "sequence"):
            meds = [r["configs"][key][name]["median_us"] for r in runs]
            rec[name + "_us"] = {"median": statistics.median(meds), "min": min(meds),
                                 "max": max(meds)}
        fu, sq = rec["fused_us"], rec["sequence_us"]
        rec["saved_us"] = sq["median"] - fu["median"]
        spread = max(fu["max"] - fu["min"], sq["max"] - sq["min"])
        rec["ahead"] = bool(rec["saved_us"] > spread)  # below by more than both sides' spread
        rec["routed_to_sequence"] = runs[0]["configs"][key]["routed_to_sequence"]
        results[key] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/collect_arrive_bench.py", "runs": RUNS, "reps_per_run": REPS,
                   "device": runs[0]["device"], "parent_collect_bench_us": PARENT_US,
                   "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
