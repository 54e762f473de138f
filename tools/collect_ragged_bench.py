"""Measure the ragged collection finish (bk_collect_finish_ragged) against the
ways there were to get finishes of mixed (n, f) over one collection, and
against the uniform entry where the problems happen to share one shape.

    python tools/collect_ragged_bench.py [--out profiles/r11/collect_ragged_bench.json]

Workloads (fp64), each in a child process of its own under a time limit, at
batch = 2, 4, 8, 16, 64, 256:

  mixed      a 200-row collection at d = 7,850; n_b uniform in 28..100, f_b
             uniform in floor(0.3 n_b)..floor(0.5 n_b), random subsets:
               ragged   one bk_collect_finish_ragged call
               loop     bk_collect_finish once per problem
               grouped  one bk_collect_finish_batch call per distinct (n, f),
                        the problems sorted into groups ahead of the clock
  uniform_B  the same collection, every problem 100 rows, f = 30:
               ragged against batched (one bk_collect_finish_batch call)
  uniform_A  a 10-row collection at d = 25, every problem its 10 rows in a
             random order, f = 2: ragged against batched

All forms of a workload run in the same process on the same context.  One
sample is the wall-clock time around `iters` back-to-back calls (every form is
synchronous), divided by iters x batch.  The forms alternate sample by sample; a
run is `reps` samples of each, three runs; reported is the median of the runs'
medians with the min..max of those medians.  A comparison's spread is the
larger (max - min) of the two forms compared: `below_*` says the ragged median
is below the other form's by more than that, `within_batched` that it is within
it.  The ragged outputs are compared bitwise with the loop's (mixed) or the
uniform entry's once per batch size.  A separate pass per form, 20 calls under
bk_timing_enable, records the HIP-event time of its launches and copies per
problem (`device_events_us`): what is left of the wall clock is the host's.
Not a pass/fail gate; prints one JSON line
per workload and writes them all.
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

WORKLOADS = {"mixed": 200, "uniform_B": 150, "uniform_A": 120}  # time limit, s
BATCHES = (2, 4, 8, 16, 64, 256)
RUNS = 3


def run_workload(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    eng = Engine(0)
    rng = np.random.default_rng(20261019)
    rows, d = (10, 25) if tag == "uniform_A" else (200, 7850)
    # rows as a federated round's: a common direction plus noise, a shifted cluster
    R = 0.01 * rng.standard_normal(d) + 1e-3 * rng.standard_normal((rows, d))
    R[: rows // 5] += 0.05 * rng.standard_normal(d)
    R = np.ascontiguousarray(R[rng.permutation(rows)])
    eng.collect_begin(rows, d, np.float64)
    for i in range(0, rows, 25):
        eng.collect_add([R[r] for r in range(i, min(rows, i + 25))])
    BMAX = max(BATCHES)
    if tag == "mixed":
        ns = rng.integers(28, 101, size=BMAX)
        fs = np.array([rng.integers(int(0.3 * n), int(0.5 * n) + 1) for n in ns], dtype=np.int64)
    elif tag == "uniform_B":
        ns, fs = np.full(BMAX, 100), np.full(BMAX, 30, dtype=np.int64)
    else:
        ns, fs = np.full(BMAX, 10), np.full(BMAX, 2, dtype=np.int64)
    ns = ns.astype(np.int64)
    orders = [rng.choice(rows, size=int(n), replace=False).astype(np.int64) for n in ns]
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(ns - fs)]).astype(np.int64)
    packed = np.ascontiguousarray(np.concatenate(orders))
    # host outputs, allocated once: [ragged, the reference form, grouped]
    hout = [(np.empty(int(so[-1]), np.int64), np.empty(int(off[-1]), np.float64),
             np.empty((BMAX, d), np.float64)) for _ in range(3)]
    mo = np.zeros(BMAX, dtype=np.int64)
    mo1 = ctypes.c_int64(0)

    def ragged(B):
        o = hout[0]
        _lib.check(L.bk_collect_finish_ragged(eng.ctx, packed.ctypes.data, off.ctypes.data,
                                              fs.ctypes.data, B, o[0].ctypes.data, mo.ctypes.data,
                                              o[1].ctypes.data, o[2].ctypes.data))

    def loop(B):
        o = hout[1]
        for b in range(B):
            _lib.check(L.bk_collect_finish(eng.ctx, orders[b].ctypes.data, int(ns[b]), int(fs[b]),
                                           o[0][so[b]:].ctypes.data, ctypes.addressof(mo1),
                                           o[1][off[b]:].ctypes.data, o[2][b].ctypes.data))

    def batched(B):  # uniform workloads: the orders are one B x n array already
        o = hout[1]
        _lib.check(L.bk_collect_finish_batch(eng.ctx, packed.ctypes.data, B, int(ns[0]), int(fs[0]),
                                             o[0].ctypes.data, ctypes.addressof(mo1),
                                             o[1].ctypes.data, o[2].ctypes.data))

    groups = {}  # B -> [(n, f, count, orders count x n, outputs)], built ahead of the clock

    def grouping(B):
        if B not in groups:
            by = {}
            for b in range(B):
                by.setdefault((int(ns[b]), int(fs[b])), []).append(b)
            groups[B] = [(n, f, len(bs), np.ascontiguousarray(np.stack([orders[b] for b in bs])),
                          np.empty((len(bs), n - f), np.int64), np.empty((len(bs), n), np.float64),
                          np.empty((len(bs), d), np.float64)) for (n, f), bs in sorted(by.items())]
        return groups[B]

    def grouped(B):
        for n, f, cnt, o, sel, sc, mean in grouping(B):
            _lib.check(L.bk_collect_finish_batch(eng.ctx, o.ctypes.data, cnt, n, f, sel.ctypes.data,
                                                 ctypes.addressof(mo1), sc.ctypes.data,
                                                 mean.ctypes.data))

    if tag == "mixed":
        forms = (("ragged", ragged), ("loop", loop), ("grouped", grouped))
    else:
        forms = (("ragged", ragged), ("batched", batched))

    def sample(call, B, iters):
        t0 = time.perf_counter()
        for _ in range(iters):
            call(B)
        return (time.perf_counter() - t0) * 1e6 / (iters * B)  # us per problem

    def summary(meds):
        return {"median_us": statistics.median(meds), "min_us": min(meds), "max_us": max(meds)}

    def spread(a, b):
        return max(a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])

    out = {"workload": tag, "d": d, "dtype": "float64", "collected_rows": rows, "runs": RUNS,
           "device": torch.cuda.get_device_name(0), "curve": []}
    for B in BATCHES:
        iters = max(1, 64 // B)
        reps = 15 if B <= 16 else 7 if B <= 64 else 5
        for _, call in forms:
            call(B)
        ends = (int(so[B]), int(off[B]), B)
        bitwise = all(np.array_equal(hout[0][q][:ends[q]].view(np.int64),
                                     hout[1][q][:ends[q]].view(np.int64)) for q in range(3))
        for _ in range(2):  # warm every form
            for _, call in forms:
                sample(call, B, iters)
        meds = {name: [] for name, _ in forms}
        for _ in range(RUNS):
            ts = {name: [] for name, _ in forms}
            for _ in range(reps):
                for name, call in forms:
                    ts[name].append(sample(call, B, iters))
            for name in ts:
                meds[name].append(statistics.median(ts[name]))
        row = {"batch": B, "iters": iters, "reps": reps, "bitwise_equal_to_reference": bool(bitwise)}
        for name in meds:
            row[name] = summary(meds[name])
        # where the time goes, in a pass of its own (the events slow the host):
        # HIP events around the launches and the copies, us per problem
        row["device_events_us"] = {}
        for name, call in forms:
            eng.timing_enable(True)
            try:
                for _ in range(20):
                    call(B)
                t = eng.timing_read()
            finally:
                eng.timing_enable(False)
            row["device_events_us"][name] = {
                k: {"per_problem_us": v["total_ms"] * 1e3 / (20 * B), "launches_per_call": v["count"] / 20}
                for k, v in t.items()}
        rg = row["ragged"]
        if tag == "mixed":
            row["distinct_shapes"] = len(grouping(B))
            for other in ("loop", "grouped"):
                sp = spread(rg, row[other])
                row["spread_vs_%s_us" % other] = sp
                row["speedup_vs_%s" % other] = row[other]["median_us"] / rg["median_us"]
                row["below_%s" % other] = rg["median_us"] < row[other]["median_us"] - sp
        else:
            sp = spread(rg, row["batched"])
            row["spread_vs_batched_us"] = sp
            row["ratio_to_batched"] = rg["median_us"] / row["batched"]["median_us"]
            row["within_batched"] = abs(rg["median_us"] - row["batched"]["median_us"]) <= sp
        out["curve"].append(row)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "r11", "collect_ragged_bench.json"))
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="(child) measure this one only")
    ap.add_argument("--workloads", default="mixed,uniform_B,uniform_A",
                    help="comma-separated workloads (default: all three)")
    args = ap.parse_args()
    if args.workload:
        run_workload(args.workload)
        return 0
    tags = [t for t in args.workloads.split(",") if t]
    if any(t not in WORKLOADS for t in tags):
        ap.error("unknown workload in --workloads (have %s)" % ",".join(sorted(WORKLOADS)))
    results = []
    for tag in tags:
        # a fresh child per workload, under its own time limit; a failed step ends the run
        r = subprocess.run(["timeout", "-k", "10", str(WORKLOADS[tag]), sys.executable,
                            os.path.abspath(__file__), "--workload", tag], stdout=subprocess.PIPE,
                           text=True)
        if r.returncode != 0:
            print("workload %s failed with status %d" % (tag, r.returncode), file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/collect_ragged_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
