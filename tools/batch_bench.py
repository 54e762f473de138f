"""Measure the batched entry (bk_multikrum_batch_device) against a loop of
bk_multikrum_device over the same problems.

    python tools/batch_bench.py [--out profiles/r09/batch_bench.json] [--shapes A,B]

Per shape (B: 100 x 7,850, f = 50; A: 10 x 25, f = 5; fp64, device-resident,
every problem its own synthetic batch), in a child process of its own under a
time limit, for batch = 1, 2, 4, 8, 16, 64, 256: the per-problem time of the
batched entry and of the loop, both in the same process on the same stream.
One sample is the HIP-event time around `iters` back-to-back calls (the loop:
iters x batch single calls), divided by iters x batch.  The two alternate
sample by sample; a run is `reps` samples of each, three runs; reported is the
median of the runs' medians with the min..max of those medians (the run-to-run
spread the comparison has to clear).  The outputs of the two are compared
bitwise once per batch size.
Not a pass/fail gate; prints one JSON line per shape and writes them all.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = {"A": (10, 25, 5, 240), "B": (100, 7850, 50, 420)}  # n, d, f, limit s
BATCHES = (1, 2, 4, 8, 16, 64, 256)
RUNS, REPS = 3, 15


def run_shape(tag):
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    n, d, f, _ = SHAPES[tag]
    m = n - f
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    BMAX = max(BATCHES)
    X = torch.empty((BMAX, n, d), dtype=torch.float64, device="cuda")
    for b in range(BMAX):
        eng.synth_fill_ptr(X.data_ptr() + b * n * d * 8, _lib.BK_F64, n, d, d, 0, d,
                           20261019 + b, f // 2)
    outs = [(torch.empty(BMAX * m, dtype=torch.int64, device="cuda"),
             torch.empty(BMAX * n, dtype=torch.float64, device="cuda"),
             torch.empty(BMAX * d, dtype=torch.float64, device="cuda")) for _ in range(2)]
    eng.synchronize()

    def batched(B, o):
        eng.multikrum_batch_device_ptr(X.data_ptr(), _lib.BK_F64, B, n, d, d, n * d, f,
                                       o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())

    def loop(B, o):
        for b in range(B):
            eng.multikrum_device_ptr(X.data_ptr() + b * n * d * 8, _lib.BK_F64, n, d, d, f,
                                     o[0].data_ptr() + 8 * b * m, o[1].data_ptr() + 8 * b * n,
                                     o[2].data_ptr() + 8 * b * d)

    def sample(call, B, o, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            call(B, o)
        b.record(stream)
        eng.synchronize()
        return a.elapsed_time(b) * 1e3 / (iters * B)  # us per problem

    def summary(meds):
        return {"median_us": statistics.median(meds), "min_us": min(meds), "max_us": max(meds)}

    out = {"shape": tag, "n": n, "d": d, "f": f, "dtype": "float64", "runs": RUNS, "reps": REPS,
           "device": torch.cuda.get_device_name(0), "curve": []}
    for B in BATCHES:
        iters = max(1, 32 // B)
        batched(B, outs[0])
        loop(B, outs[1])
        eng.synchronize()
        bitwise = all(torch.equal(outs[0][q][:B * w].view(torch.int64),
                                  outs[1][q][:B * w].view(torch.int64))
                      for q, w in ((0, m), (1, n), (2, d)))
        for _ in range(3):  # warm both
            sample(batched, B, outs[0], iters)
            sample(loop, B, outs[1], iters)
        mb, ml = [], []
        for _ in range(RUNS):
            tb, tl = [], []
            for _ in range(REPS):
                tb.append(sample(batched, B, outs[0], iters))
                tl.append(sample(loop, B, outs[1], iters))
            mb.append(statistics.median(tb))
            ml.append(statistics.median(tl))
        row = {"batch": B, "iters": iters, "bitwise_equal": bool(bitwise),
               "batched": summary(mb), "loop": summary(ml)}
        row["speedup"] = row["loop"]["median_us"] / row["batched"]["median_us"]
        # batching pays when the slowest batched run beats the fastest loop run
        row["clears_spread"] = row["batched"]["max_us"] < row["loop"]["min_us"]
        out["curve"].append(row)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "batch_bench.json"))
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(child) measure this shape only")
    ap.add_argument("--shapes", default="B,A", help="comma-separated shapes (default: B,A)")
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape)
        return 0
    tags = [t for t in args.shapes.split(",") if t]
    if any(t not in SHAPES for t in tags):
        ap.error("unknown shape in --shapes (have %s)" % ",".join(sorted(SHAPES)))
    results = []
    for tag in tags:
        # a fresh child per shape, under its own time limit; a failed step ends the run
        r = subprocess.run(["timeout", "-k", "10", str(SHAPES[tag][3]), sys.executable,
                            os.path.abspath(__file__), "--shape", tag], stdout=subprocess.PIPE,
                           text=True)
        if r.returncode != 0:
            print("shape %s failed with status %d" % (tag, r.returncode), file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/batch_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
