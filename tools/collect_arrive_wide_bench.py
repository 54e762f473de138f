"""Measure the fused wide last arrival (bk_set_collect_wide_arrive,
k_collect_arrive_wide) against the sequence the same entry runs with the switch
off (the row's copy, k_border, k_border_reduce, then k_collect_wide and its wait).

    python tools/collect_arrive_wide_bench.py [--out profiles/r23/collect_arrive_wide_bench.json]

Per shape (100 x 163,850 fp64 and fp32, 100 x 259,770 fp64 without the mean, 100
x 40,000 fp64), row source (pinned, device) and output set (with and without the
mean), in ONE process on one GPU with the wide path on: every row but the last
is collected and the stream idle (the verifier waiting for its last peer); then
the wall clock around the C call, from the start of the last arrival to the
verdict's return -- bk_collect_add_finish with the switch on and with it off on
the same rows, alternating.  collect_stats() must show the path each took (a
call with the mean past BK_COLLECT_WIDE_MEAN_MAX_D is outside the wide range:
`routed_to_sequence`, both sides then run the same launches), and the two
verdicts must agree bitwise.  Three runs (a child process each, under its own
time limit, behind one more that only warms the machine up and is not counted);
every figure is the median of the runs' medians with [min .. max] over the
runs.  `ahead` says whether the fused median is below the sequence's by more
than both sides' spread.  Not a pass/fail gate; prints one JSON line per run and
writes the summary.
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

# tag: (n, d, f, dtype, output sets)
SHAPES = {"cnn_f64": (100, 163850, 30, "f64", (True, False)),
          "cnn_f32": (100, 163850, 30, "f32", (True, False)),
          "cnn2_f64": (100, 259770, 30, "f64", (False,)),
          "d40000_f64": (100, 40000, 30, "f64", (True, False))}
MEAN_MAX_D = 165888  # bk.h BK_COLLECT_WIDE_MEAN_MAX_D
REPS, RUNS, LIMIT = 20, 3, 280
FUSED = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 1}
SEQUENCE = {"border": 1, "border_reduce": 1, "one_launch_finishes": 1, "fused_arrivals": 0}
CHAIN = {"border": 1, "border_reduce": 1, "one_launch_finishes": 0, "fused_arrivals": 0}


def run_once(only=None):
    """(child) every configuration once -> one JSON line"""
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    eng.set_collect_wide(True)
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "configs": {}}
    for tag, (n, d, f, dt, sets) in sorted(SHAPES.items()):
        if only and tag not in only:
            continue
        f64 = dt == "f64"
        es = 8 if f64 else 4
        npdt = np.float64 if f64 else np.float32
        Xd = torch.empty((n, d), dtype=torch.float64 if f64 else torch.float32, device="cuda")
        eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64 if f64 else _lib.BK_F32, n, d, d, 0, d,
                           20261021, f)
        eng.synchronize()
        Xp = Xd.cpu().pin_memory()
        m = n - f
        sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
        sc, mean = np.empty(n), np.empty(d)
        for src, X, where in (("pinned", Xp, _lib.BK_HOST_PINNED), ("device", Xd, _lib.BK_DEVICE)):
            base = X.data_ptr()

            def rows(i, k=1):
                return (ctypes.c_void_p * k)(*[base + (i + q) * d * es for q in range(k)])

            def resident():
                eng.collect_begin(n, d, npdt)
                for i in range(0, n - 1, 8):
                    k = min(8, n - 1 - i)
                    eng.collect_add_ptr(rows(i, k), k, where)
                eng.synchronize()
                return eng.collect_stats()

            for with_mean in sets:
                mp = mean.ctypes.data if with_mean else None
                last = rows(n - 1)
                routed = with_mean and d > MEAN_MAX_D

                def arrive(on):
                    eng.set_collect_wide_arrive(on, everywhere=True)  # the uncut range
                    s0 = resident()
                    t0 = time.perf_counter()
                    st = L.bk_collect_add_finish(eng.ctx, last[0], where, None, n, f, None,
                                                 sel.ctypes.data, ctypes.addressof(mo),
                                                 sc.ctypes.data, mp)
                    t1 = time.perf_counter()
                    _lib.check(st)
                    s1 = eng.collect_stats()
                    return (t1 - t0) * 1e6, {k: s1[k] - s0[k] for k in s1}

                ts = {"fused": [], "sequence": []}
                got = {}
                for r in range(REPS + 3):  # the first three of each: warm-up
                    for name, on in (("fused", True), ("sequence", False)):
                        us, took = arrive(on)
                        want = CHAIN if routed else FUSED if on else SEQUENCE
                        assert took == want, (tag, src, with_mean, name, took)
                        got[name] = (sel.copy(), sc.copy(), mean.copy() if with_mean else None)
                        if r >= 3:
                            ts[name].append(us)
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
        del Xp, Xd
    eng.set_collect_wide_arrive(False)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(child) one run")
    ap.add_argument("--only", default="", help="comma-separated shape tags (default: all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r23",
                                                  "collect_arrive_wide_bench.json"))
    args = ap.parse_args()
    only = [t for t in args.only.split(",") if t]
    if args.child:
        run_once(only)
        return 0
    runs = []
    for k in range(RUNS + 1):  # the first child warms the machine up: printed, not counted
        # a fresh child per run, under its own time limit; a failed run ends the tool
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__),
               "--child"] + (["--only", args.only] if only else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
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
        json.dump({"tool": "tools/collect_arrive_wide_bench.py", "runs": RUNS, "reps_per_run": REPS,
                   "device": runs[0]["device"], "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
