"""Measure the ragged batched entry (bk_multikrum_ragged_device) against what a
caller had before it.

    python tools/batch_ragged_bench.py [--out profiles/r14/batch_ragged_bench.json]

Everything is device-resident fp64 at d = 7,850, every problem its own
synthetic batch, in a child process per part under a time limit.

mixed    n uniform in 28..100, f uniform in ceil(0.3 n)..floor(0.5 n) (seeded),
         batch = 2, 16, 64, 256.  The ragged call against (a) a loop of
         bk_multikrum_device over the problems and (b) one
         bk_multikrum_batch_device per distinct (n, f) on a regrouped,
         already-resident copy (the regrouping is not charged to (b)).
uniform  every problem 100 x 7,850 with f = 30, and 10 x 25 with f = 2, batch =
         2, 16, 64, 256: the ragged call against bk_multikrum_batch_device --
         what the descriptor read and the segment search cost.

One sample is the HIP-event time around `iters` back-to-back calls, divided by
iters x batch (us per problem).  The competitors alternate sample by sample in
one process on one stream; a run is `reps` samples of each, three runs;
reported is the median of the runs' medians with the min..max of those medians
(the run-to-run spread a comparison has to clear).  The outputs are compared
bitwise once per batch size.  Not a pass/fail gate; prints one JSON line per
part and writes them all.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PARTS = {"mixed": 420, "uniformB": 300, "uniformA": 200}  # time limit, s
UNIFORM = {"uniformB": (100, 7850, 30), "uniformA": (10, 25, 2)}
BATCHES = (2, 16, 64, 256)
RUNS, REPS = 3, 9
D = 7850


def _summary(meds):
    return {"median_us": statistics.median(meds), "min_us": min(meds), "max_us": max(meds)}


def _measure(torch, eng, stream, B, calls, iters):
    """calls: name -> f(); alternating samples, RUNS x REPS -> name -> summary"""
    def sample(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            call()
        b.record(stream)
        eng.synchronize()
        return a.elapsed_time(b) * 1e3 / (iters * B)

    for _ in range(2):  # warm all
        for call in calls.values():
            sample(call)
    meds = {k: [] for k in calls}
    for _ in range(RUNS):
        t = {k: [] for k in calls}
        for _ in range(REPS):
            for k, call in calls.items():
                t[k].append(sample(call))
        for k in calls:
            meds[k].append(statistics.median(t[k]))
    return {k: _summary(v) for k, v in meds.items()}


def run_part(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    BMAX = max(BATCHES)
    rng = np.random.default_rng(20261020)
    if tag == "mixed":
        d = D
        ns = rng.integers(28, 101, size=BMAX)
        fs = np.array([rng.integers(math.ceil(0.3 * n), n // 2 + 1) for n in ns], dtype=np.int64)
    else:
        n0, d, f0 = UNIFORM[tag]
        ns = np.full(BMAX, n0, dtype=np.int64)
        fs = np.full(BMAX, f0, dtype=np.int64)
    ns = ns.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(ns - fs)]).astype(np.int64)
    X = torch.empty((int(off[-1]), d), dtype=torch.float64, device="cuda")
    for b in range(BMAX):
        eng.synth_fill_ptr(X.data_ptr() + int(off[b]) * d * 8, _lib.BK_F64, int(ns[b]), d, d, 0, d,
                           20261020 + b, int(fs[b]) // 2)

    def outs():
        return (torch.empty(int(so[-1]), dtype=torch.int64, device="cuda"),
                torch.empty(int(off[-1]), dtype=torch.float64, device="cuda"),
                torch.empty(BMAX * d, dtype=torch.float64, device="cuda"))

    o_r, o_l, o_g = outs(), outs(), outs()
    eng.synchronize()

    def ragged(B):
        eng.multikrum_ragged_device_ptr(X.data_ptr(), _lib.BK_F64, off[:B + 1], fs[:B], d, d,
                                        o_r[0].data_ptr(), o_r[1].data_ptr(), o_r[2].data_ptr())

    def loop(B):
        for b in range(B):
            eng.multikrum_device_ptr(X.data_ptr() + int(off[b]) * d * 8, _lib.BK_F64, int(ns[b]), d,
                                     d, int(fs[b]), o_l[0].data_ptr() + 8 * int(so[b]),
                                     o_l[1].data_ptr() + 8 * int(off[b]),
                                     o_l[2].data_ptr() + 8 * b * d)

    def same(a, b, B):
        return all(torch.equal(a[q][:w].view(torch.int64), b[q][:w].view(torch.int64))
                   for q, w in ((0, int(so[B])), (1, int(off[B])), (2, B * d)))

    out = {"part": tag, "d": d, "dtype": "float64", "runs": RUNS, "reps": REPS,
           "device": torch.cuda.get_device_name(0), "curve": []}
    for B in BATCHES:
        iters = max(1, 32 // B)
        calls = {"ragged": lambda: ragged(B), "loop": lambda: loop(B)}
        row = {"batch": B, "iters": iters}
        if tag == "mixed":
            # (b): the problems regrouped by (n, f), each group contiguous in a
            # resident copy of its own; its outputs are the groups' own
            groups = {}
            for b in range(B):
                groups.setdefault((int(ns[b]), int(fs[b])), []).append(b)
            row["distinct_shapes"] = len(groups)
            order = [b for g in groups.values() for b in g]
            Xg = torch.cat([X[int(off[b]):int(off[b + 1])] for b in order])
            plan, r0, s0, b0 = [], 0, 0, 0
            for (n, f), g in groups.items():
                plan.append((n, f, len(g), r0, s0, b0))
                r0, s0, b0 = r0 + n * len(g), s0 + (n - f) * len(g), b0 + len(g)

            def grouped():
                for n, f, cnt, r, s, q in plan:
                    eng.multikrum_batch_device_ptr(Xg.data_ptr() + r * d * 8, _lib.BK_F64, cnt, n,
                                                   d, d, n * d, f, o_g[0].data_ptr() + 8 * s,
                                                   o_g[1].data_ptr() + 8 * r,
                                                   o_g[2].data_ptr() + 8 * q * d)

            calls["grouped"] = grouped
        else:
            n0, _, f0 = UNIFORM[tag]

            def batched():
                eng.multikrum_batch_device_ptr(X.data_ptr(), _lib.BK_F64, B, n0, d, d, n0 * d, f0,
                                               o_g[0].data_ptr(), o_g[1].data_ptr(),
                                               o_g[2].data_ptr())

            calls["batched"] = batched
        for call in calls.values():
            call()
        eng.synchronize()
        row["bitwise_equal_loop"] = bool(same(o_r, o_l, B))
        if tag != "mixed":
            row["bitwise_equal_batched"] = bool(same(o_r, o_g, B))
        row.update(_measure(torch, eng, stream, B, calls, iters))
        others = [k for k in calls if k != "ragged"]
        for k in others:
            row["speedup_vs_" + k] = row[k]["median_us"] / row["ragged"]["median_us"]
        # ahead of a competitor when the slowest ragged run beats its fastest run
        row["clears_spread"] = {k: row["ragged"]["max_us"] < row[k]["min_us"] for k in others}
        out["curve"].append(row)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14", "batch_ragged_bench.json"))
    ap.add_argument("--part", choices=sorted(PARTS), help="(child) measure this part only")
    ap.add_argument("--parts", default="mixed,uniformB,uniformA")
    args = ap.parse_args()
    if args.part:
        run_part(args.part)
        return 0
    tags = [t for t in args.parts.split(",") if t]
    if any(t not in PARTS for t in tags):
        ap.error("unknown part in --parts (have %s)" % ",".join(sorted(PARTS)))
    results = []
    for tag in tags:
        # a fresh child per part, under its own time limit; a failed step ends the run
        r = subprocess.run(["timeout", "-k", "10", str(PARTS[tag]), sys.executable,
                            os.path.abspath(__file__), "--part", tag], stdout=subprocess.PIPE,
                           text=True)
        if r.returncode != 0:
            print("part %s failed with status %d" % (tag, r.returncode), file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/batch_ragged_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
