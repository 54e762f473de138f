"""Measure the noised incremental collection (bk_collect_add_noised) against the
two routes there were to the same verdict for updates that carry Delta and
Noise separately.

    python tools/collect_noised_bench.py [--out profiles/r13/collect_noised_bench.json] [--shapes B,D]

Per shape (B: 100 x 7,850, f = 30; D: 512 x 1,048,576, f = 153; fp64), in a
child process of its own under a time limit, with the rows in pinned and in
pageable host memory and k = 1 and k = 2 noise vectors per update, all in the
same process on the same context:

  noised      bk_collect_add_noised per arrival (the noise added on the device)
  host_noise  numpy delta + mean of the noise vectors on a host core into a
              pinned row, then bk_collect_add(BK_HOST_PINNED) per arrival
  batch       bk_multikrum_noised(BK_HOST_PINNED) over the whole batch (always
              from the pinned copy)

For the two per-arrival routes one run fills the collection `fills` times and
takes
  (a) add: the wall time of one add, to the entry's return (call_us) and to an
      idle stream (folded_us: bk_synchronize behind it), the median over the
      arrivals 0 .. n-2 of the run's fills;
  (b) last_to_verdict_ms: from the start of the last add (on an idle stream) to
      the return of bk_collect_finish (scores and mean requested), the median
      over the run's fills.
Three runs; reported is the median of the runs' medians with their min and max
(the run-to-run spread a comparison has to clear).  batch is the wall time of
the call, the same statistics.  The three routes' selections are compared, and
the two collections' means bitwise.  Not a pass/fail gate; prints one JSON line
per shape and writes them all.
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

SHAPES = {"B": (100, 7850, 30, 5, 300), "D": (512, 1048576, 153, 1, 900)}  # n, d, f, fills, limit s
KS = (1, 2)
KMAX = max(KS)
RUNS = 3


def run_shape(tag):
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    n, d, f, fills, _ = SHAPES[tag]
    m = n - f
    L = _lib.lib()
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    Xd = torch.empty((n, d), dtype=torch.float64, device="cuda")
    eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64, n, d, d, 0, d, 20261019, f)
    eng.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(20261020)
    Nd = torch.randn((n, KMAX, d), dtype=torch.float64, device="cuda", generator=gen) * 1e-4
    torch.cuda.synchronize()
    X = {"pageable": Xd.cpu(), "pinned": Xd.cpu().pin_memory()}
    Nz = {"pageable": Nd.cpu(), "pinned": Nd.cpu().pin_memory()}
    del Xd, Nd
    torch.cuda.empty_cache()
    scratch = torch.empty(d, dtype=torch.float64).pin_memory()
    scratch_np, tmp = scratch.numpy(), np.empty(d)
    scratch_ptr = (ctypes.c_void_p * 1)(scratch.data_ptr())
    sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
    sc, mean = np.empty(n), np.empty(d)

    def finish():
        _lib.check(L.bk_collect_finish(eng.ctx, None, n, f, sel.ctypes.data, ctypes.addressof(mo),
                                       sc.ctypes.data, mean.ctypes.data))

    def make_noised(mem, k):
        xb, nb = X[mem].data_ptr(), Nz[mem].data_ptr()
        where = _lib.BK_HOST_PINNED if mem == "pinned" else _lib.BK_HOST
        ptrs = [((ctypes.c_void_p * 1)(xb + i * d * 8),
                 (ctypes.c_void_p * k)(*[nb + (i * KMAX + j) * d * 8 for j in range(k)]))
                for i in range(n)]

        def add(i):
            _lib.check(L.bk_collect_add_noised(eng.ctx, ptrs[i][0], ptrs[i][1], k, 1, where, None))
        return add

    def make_host_noise(mem, k):
        xn, nn = X[mem].numpy(), Nz[mem].numpy()

        def add(i):
            # the entry's bits: (0 + v_0) / 1 = v_0; ((0 + v_0) + v_1) / 2 = (v_0 + v_1) * 0.5
            if k == 1:
                np.add(xn[i], nn[i, 0], out=scratch_np)
            else:
                np.add(nn[i, 0], nn[i, 1], out=tmp)
                np.multiply(tmp, 0.5, out=tmp)
                np.add(xn[i], tmp, out=scratch_np)
            _lib.check(L.bk_collect_add(eng.ctx, scratch_ptr, 1, _lib.BK_HOST_PINNED, None))
        return add

    def batch(k):
        # vector j of update i at noise + (i k + j) noise_ld: the first k of each update's KMAX
        _lib.check(L.bk_multikrum_noised(eng.ctx, ctypes.c_void_p(X["pinned"].data_ptr()), d,
                                         ctypes.c_void_p(Nz["pinned"].data_ptr()), k,
                                         d * KMAX // k, _lib.BK_HOST_PINNED, n, d, f,
                                         sel.ctypes.data, ctypes.addressof(mo), sc.ctypes.data,
                                         mean.ctypes.data, None, d))

    def one_fill(add, call, folded):
        eng.collect_begin(n, d, np.float64)
        eng.synchronize()
        for i in range(n - 1):
            t0 = time.perf_counter()
            add(i)
            t1 = time.perf_counter()
            eng.synchronize()
            t2 = time.perf_counter()
            call.append((t1 - t0) * 1e6)
            folded.append((t2 - t0) * 1e6)
        t0 = time.perf_counter()
        add(n - 1)
        finish()
        return (time.perf_counter() - t0) * 1e3

    def spread(vals):
        return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}

    def measure(add):
        one_fill(add, [], [])  # warm: buffers, code objects
        runs = {"call_us": [], "folded_us": [], "last_to_verdict_ms": []}
        for _ in range(RUNS):
            call, folded, last = [], [], []
            for _ in range(fills):
                last.append(one_fill(add, call, folded))
            runs["call_us"].append(statistics.median(call))
            runs["folded_us"].append(statistics.median(folded))
            runs["last_to_verdict_ms"].append(statistics.median(last))
        return {key: spread(v) for key, v in runs.items()}

    out = {"shape": tag, "n": n, "d": d, "f": f, "dtype": "float64", "runs": RUNS, "fills": fills,
           "device": torch.cuda.get_device_name(0), "configs": []}
    for k in KS:
        batch(k)
        ts = []
        for _ in range(RUNS):
            one = []
            for _ in range(max(1, fills)):
                t0 = time.perf_counter()
                batch(k)
                one.append((time.perf_counter() - t0) * 1e3)
            ts.append(statistics.median(one))
        batch_ms = spread(ts)
        batch_sel = sel.copy()
        for mem in ("pinned", "pageable"):
            row = {"rows": mem, "k": k, "batch_ms": batch_ms}
            row["noised"] = measure(make_noised(mem, k))
            nsel, nmean = sel.copy(), mean.copy()
            row["host_noise"] = measure(make_host_noise(mem, k))
            row["same_selection"] = bool(np.array_equal(nsel, sel) and
                                         np.array_equal(nsel, batch_sel))
            row["mean_bitwise_equal"] = bool(np.array_equal(nmean.view(np.int64),
                                                            mean.view(np.int64)))
            a, b = row["noised"], row["host_noise"]
            row["add_folded_ratio_to_host_noise"] = (a["folded_us"]["median"] /
                                                     b["folded_us"]["median"])
            row["last_to_verdict_ratio_to_host_noise"] = (a["last_to_verdict_ms"]["median"] /
                                                          b["last_to_verdict_ms"]["median"])
            row["last_to_verdict_ratio_to_batch"] = (a["last_to_verdict_ms"]["median"] /
                                                     batch_ms["median"])
            # ahead only when the slowest noised run beats the fastest run of the other route
            row["add_clears_host_noise_spread"] = a["folded_us"]["max"] < b["folded_us"]["min"]
            row["last_clears_host_noise_spread"] = (a["last_to_verdict_ms"]["max"] <
                                                    b["last_to_verdict_ms"]["min"])
            out["configs"].append(row)
            print("%s: %s rows, k = %d measured" % (tag, mem, k), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(REPO, "profiles", "r13", "collect_noised_bench.json"))
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(child) measure this shape only")
    ap.add_argument("--shapes", default="B,D", help="comma-separated shapes (default: B,D)")
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
        r = subprocess.run(["timeout", "-k", "10", str(SHAPES[tag][4]), sys.executable,
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
        json.dump({"tool": "tools/collect_noised_bench.py", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
