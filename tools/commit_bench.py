"""bk_commit_* timings on the MI355X -> profiles/r27/commit_bench.json.

    python tools/commit_bench.py [--out profiles/r27/commit_bench.json] [--no-host]

Shapes: creditcard d = 25, mnist d = 7,850, lfw d = 104,916, poly_size 10,
total_shares 20, precision 4, deltas ~ N(0, 0.1).  Entries: bk_commit_msm alone
(host scalars), bk_commit_generate with all three outputs (host delta) and
bk_commit_set_key.  Each figure is the median [min .. max] of three runs, a run
the mean of `reps` back-to-back calls after one warm-up call.

The grid of k_commit_msm (BK_COMMIT_MSM_TERMS terms per thread) is measured at
1, 4 (the default) and 16.

The CPU baseline is the host build of bk_bn256.h (tools/commit_host.cpp) on this
machine, 1 and 16 threads: the same windowed algorithm, double-and-add on |v|,
and double-and-add on the scalar reduced modulo the order as the reference
multiplies.  It is NOT kyber's Go code; parity with Go is unpinned.
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

SHAPES = [("creditcard", 25), ("mnist", 7850), ("lfw", 104916)]
P, T, PREC = 10, 20, 4


def key_bytes(count):
    import commit_ref as C
    out, a = bytearray(), C.G
    for _ in range(count):
        out += C.marshal(a)
        a = C.double(a)
    return bytes(out)


def three(fn, reps):
    fn()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        runs.append((time.perf_counter() - t0) / reps * 1e3)
    return {"median_ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs),
            "reps": reps}


def gpu(key, terms):
    if terms is None:
        os.environ.pop("BK_COMMIT_MSM_TERMS", None)
    else:
        os.environ["BK_COMMIT_MSM_TERMS"] = str(terms)
    from biscotti_amd.krum import Engine
    eng = Engine(0)
    out = {}
    try:
        for name, d in SHAPES:
            raw = key[:64 * d]
            reps = 20 if d < 10000 else 3
            rec = {"d": d}
            if terms is None:
                rec["set_key"] = three(lambda: eng.commit_set_key(raw), max(1, reps // 4))
            else:
                eng.commit_set_key(raw)
            delta = np.random.default_rng(d).normal(0.0, 0.1, size=d)
            q = np.array([int(v * 10 ** PREC) for v in delta], dtype=np.int64)
            rec["msm"] = three(lambda: eng.commit_msm(q), reps)
            if terms is None:
                rec["generate"] = three(lambda: eng.commit_generate(delta, PREC, P, T), reps)
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
    for name, d in SHAPES:
        rec = {"d": d}
        for threads in (1, 16):
            for algo, label in ((2, "windows"), (1, "double_and_add_abs"),
                                (0, "double_and_add_reduced")):
                runs = []
                for _ in range(3 if d < 10000 else 1):
                    r = subprocess.run([exe, "bench", str(d), str(threads), str(algo), "1"],
                                       capture_output=True, text=True, check=True)
                    runs.append(float(r.stdout.split()[0]))
                rec["%s_t%d" % (label, threads)] = {"median_ms": statistics.median(runs),
                                                    "min_ms": min(runs), "max_ms": max(runs)}
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r27", "commit_bench.json"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    key = key_bytes(max(d for _, d in SHAPES))
    rec = {"poly_size": P, "total_shares": T, "precision": PREC,
           "gpu": gpu(key, None),
           "msm_terms_per_thread": {str(t): gpu(key, t) for t in (1, 16)},
           "host_msm_baseline": host(a.no_host),
           "note": "host baseline: bk_bn256.h built for the CPU, not kyber's Go; msm only"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
