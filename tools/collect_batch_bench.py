"""Measure the batched collection finish (bk_collect_finish_batch) against the
two ways there were to get many finishes over one collection.

    python tools/collect_batch_bench.py [--out profiles/r10/collect_batch_bench.json] [--shapes B,A]

Per shape (B: 100 x 7,850, f = 30; A: 10 x 25, f = 2; fp64), in a child process
of its own under a time limit: a 200-row collection, and for batch = 1, 2, 4,
8, 16, 64, 256 random subsets of n of its rows, the per-problem time of

  batched       bk_collect_finish_batch on the batch x n slot numbers
  loop          bk_collect_finish once per problem, the same orders
  packed_host   bk_multikrum_batch on the materialised subsets (batch x n x d
                host rows), the upload included
  packed_dev    bk_multikrum_batch_device on the same subsets already on the
                device, then bk_synchronize: the upload excluded (its outputs
                stay on the device, the other three copy theirs to the host)

all in the same process on the same context.  One sample is the wall-clock time
around `iters` back-to-back calls (every form is synchronous), divided by
iters x batch.  The forms alternate sample by sample; a run is `reps` samples of
each, three runs; reported is the median of the runs' medians with the min..max
of those medians (the run-to-run spread a comparison has to clear).  The
batched outputs are compared bitwise with the loop's once per batch size.
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

SHAPES = {"A": (10, 25, 2, 300), "B": (100, 7850, 30, 540)}  # n, d, f, limit s
BATCHES = (1, 2, 4, 8, 16, 64, 256)
ROWS = 200
RUNS = 3


def run_shape(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    n, d, f, _ = SHAPES[tag]
    m = n - f
    L = _lib.lib()
    eng = Engine(0)
    rng = np.random.default_rng(20261019)
    # rows as a federated round's: a common direction plus noise, a shifted cluster
    R = 0.01 * rng.standard_normal(d) + 1e-3 * rng.standard_normal((ROWS, d))
    R[: ROWS // 5] += 0.05 * rng.standard_normal(d)
    R = np.ascontiguousarray(R[rng.permutation(ROWS)])
    eng.collect_begin(ROWS, d, np.float64)
    for i in range(0, ROWS, 25):
        eng.collect_add([R[r] for r in range(i, i + 25)])
    BMAX = max(BATCHES)
    orders = np.stack([rng.choice(ROWS, size=n, replace=False) for _ in range(BMAX)]).astype(np.int64)
    packed = np.ascontiguousarray(R[orders])  # BMAX x n x d: the materialised subsets
    dpacked = torch.from_numpy(packed).cuda()
    dout = (torch.empty(BMAX * m, dtype=torch.int64, device="cuda"),
            torch.empty(BMAX * n, dtype=torch.float64, device="cuda"),
            torch.empty(BMAX * d, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    # host outputs, allocated once: [batched, loop, packed_host]
    hout = [(np.empty((BMAX, m), np.int64), np.empty((BMAX, n), np.float64),
             np.empty((BMAX, d), np.float64)) for _ in range(3)]
    mo = ctypes.c_int64(0)

    def batched(B):
        o = hout[0]
        _lib.check(L.bk_collect_finish_batch(eng.ctx, orders.ctypes.data, B, n, f, o[0].ctypes.data,
                                             ctypes.addressof(mo), o[1].ctypes.data,
                                             o[2].ctypes.data))

    def loop(B):
        o = hout[1]
        for b in range(B):
            _lib.check(L.bk_collect_finish(eng.ctx, orders[b].ctypes.data, n, f,
                                           o[0][b].ctypes.data, ctypes.addressof(mo),
                                           o[1][b].ctypes.data, o[2][b].ctypes.data))

    def packed_host(B):
        o = hout[2]
        _lib.check(L.bk_multikrum_batch(eng.ctx, packed.ctypes.data, _lib.BK_HOST, _lib.BK_F64, B, n,
                                        d, d, n * d, f, o[0].ctypes.data, ctypes.addressof(mo),
                                        o[1].ctypes.data, o[2].ctypes.data))

    def packed_dev(B):
        eng.multikrum_batch_device_ptr(dpacked.data_ptr(), _lib.BK_F64, B, n, d, d, n * d, f,
                                       dout[0].data_ptr(), dout[1].data_ptr(), dout[2].data_ptr())
        eng.synchronize()

    forms = (("batched", batched), ("loop", loop), ("packed_host", packed_host),
             ("packed_dev", packed_dev))

    def sample(call, B, iters):
        t0 = time.perf_counter()
        for _ in range(iters):
            call(B)
        return (time.perf_counter() - t0) * 1e6 / (iters * B)  # us per problem

    def summary(meds):
        return {"median_us": statistics.median(meds), "min_us": min(meds), "max_us": max(meds)}

    out = {"shape": tag, "n": n, "d": d, "f": f, "dtype": "float64", "collected_rows": ROWS,
           "runs": RUNS, "device": torch.cuda.get_device_name(0), "curve": []}
    for B in BATCHES:
        iters = max(1, 32 // B)
        reps = 15 if B <= 16 else 7 if B <= 64 else 5
        for _, call in forms:
            call(B)
        bitwise = all(np.array_equal(hout[0][q][:B].view(np.int64), hout[1][q][:B].view(np.int64))
                      for q in range(3))
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
        row = {"batch": B, "iters": iters, "reps": reps, "bitwise_equal_to_loop": bool(bitwise)}
        for name in meds:
            row[name] = summary(meds[name])
        bm = row["batched"]
        row["speedup_vs_loop"] = row["loop"]["median_us"] / bm["median_us"]
        # batching pays when the slowest batched run beats the fastest run of the loop
        row["clears_loop_spread"] = bm["max_us"] < row["loop"]["min_us"]
        row["ratio_to_packed_host"] = bm["median_us"] / row["packed_host"]["median_us"]
        row["ratio_to_packed_dev"] = bm["median_us"] / row["packed_dev"]["median_us"]
        out["curve"].append(row)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "r10", "collect_batch_bench.json"))
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
        json.dump({"tool": "tools/collect_batch_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
