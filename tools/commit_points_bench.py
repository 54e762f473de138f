"""bk_commit_points_* timings on the MI355X -> profiles/r28/commit_points_bench.json.

    python tools/commit_points_bench.py [--out profiles/r28/commit_points_bench.json] [--no-host]

Shapes: creditcard (d = 25, 3 chunks), mnist (785 chunks), lfw (10,492 chunks),
held = 5, node lists of 35 and 100 parts.  Points are drawn per (part, point
number) from 64 valid points.  Host arrays in and out.  Each figure is the
median [min .. max] of three runs, a run the mean of `reps` back-to-back calls
after one warm-up call.

Timed: one bk_commit_points_add (with the begin that frees its slot, and that
begin alone); one bk_commit_points_sum at lanes = 0 (the library's choice) and at
each forced lane-group width, the widths' runs alternating.  The inversion A/B
of DESIGN.md §5x (profiles/r28/commit_points_inversion_ab.json) was taken with
this tool on a build that still had the product tree.

The CPU baseline is the host build of bk_bn256.h (tools/commit_host.cpp sum) on
this machine, 1 and 16 threads: complete mixed additions into a Jacobian sum,
one inversion per point.  It is NOT kyber's Go code; parity with Go is unpinned.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = [("creditcard", 3), ("mnist", 785), ("lfw", 10492)]
HELD, LISTS, LANES = 5, (35, 100), (1, 2, 4, 8, 16)


def pool():
    import commit_ref as C
    pts, a = [], C.G
    for _ in range(32):
        pts += [C.marshal(a), C.marshal(C.neg(a))]
        a = C.double(a)
    return np.frombuffer(b"".join(pts), dtype=np.uint8).reshape(64, 64)


def runs_of(fns, reps):
    """Three alternating runs of each of fns: a list of {median, min, max}."""
    for fn in fns:
        fn()
    runs = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            runs[i].append((time.perf_counter() - t0) / reps * 1e3)
    return [{"median_ms": statistics.median(r), "min_ms": min(r), "max_ms": max(r), "reps": reps}
            for r in runs]


def gpu():
    from biscotti_amd.krum import Engine
    pl = pool()
    eng = Engine(0)
    out = {}
    try:
        for name, chunks in SHAPES:
            np_ = 1 + chunks * (1 + HELD)
            rng = np.random.default_rng(chunks)
            reps = 20 if chunks < 5000 else 5
            rec = {"chunks": chunks, "held": HELD, "points": np_}
            parts = []
            for _ in range(max(LISTS)):
                row = pl[rng.integers(0, 64, size=np_)]
                per = row[1:].reshape(chunks, 1 + HELD, 64)
                parts.append((row[0], per[:, 0].copy(), per[:, 1:].copy()))

            def begin():
                eng.commit_points_begin(chunks, HELD, max(LISTS))

            def add_one():  # into a store restarted each time, so the slot is free
                begin()
                eng.commit_points_add(*parts[0])

            rec["add_with_begin"], rec["begin_alone"] = runs_of([add_one, begin], reps)
            begin()
            for p in parts:
                eng.commit_points_add(*p)
            for n in LISTS:
                slots = np.arange(n, dtype=np.int64)

                def at(lanes):
                    def fn():
                        eng.commit_points_set_lanes(lanes)
                        return eng.commit_points_sum(slots)
                    return fn

                widths = (0,) + LANES
                got = [b"".join(x.tobytes() for x in at(w)()) for w in widths]
                assert all(g == got[0] for g in got), (name, n)
                rec["sum_n%d" % n] = {"lanes_%d" % w: r
                                      for w, r in zip(widths, runs_of([at(w) for w in widths], reps))}
            eng.commit_points_set_lanes(0)
            out[name] = rec
    finally:
        eng.close()
    return out


def host(no_host):
    if no_host:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="commit_host_"), "commit_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(REPO, "biscotti_amd", "csrc"),
                    os.path.join(REPO, "tools", "commit_host.cpp"), "-o", exe], check=True)
    out = {}
    for name, chunks in SHAPES:
        np_ = 1 + chunks * (1 + HELD)
        rec = {}
        for n in LISTS:
            for threads in (1, 16):
                if threads == 1 and np_ * n > 2_000_000:
                    nruns = 1
                else:
                    nruns = 3
                runs = []
                for _ in range(nruns):
                    r = subprocess.run([exe, "sum", str(np_), str(n), str(threads), "1"],
                                       capture_output=True, text=True, check=True)
                    runs.append(float(r.stdout.split()[0]))
                rec["n%d_t%d" % (n, threads)] = {"median_ms": statistics.median(runs),
                                                 "min_ms": min(runs), "max_ms": max(runs)}
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r28", "commit_points_bench.json"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    rec = {"command": "python tools/commit_points_bench.py", "held": HELD,
           "gpu": gpu(), "host_sum_baseline": host(a.no_host),
           "note": "host baseline: bk_bn256.h built for the CPU, not kyber's Go"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
