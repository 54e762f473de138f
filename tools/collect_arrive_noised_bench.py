"""Measure the noised last arrival in one launch (bk_collect_add_noised_finish)
against the two routes a verifier has without it.

    python tools/collect_arrive_noised_bench.py [--out profiles/r18/collect_arrive_noised_bench.json]

Per shape (B: 100 x 7,850 and A: 10 x 25, fp64) and setting (k in {1, 2} x
{pinned, pageable}, and device rows at k = 1), in ONE process on one GPU: every
row but the last is collected and the stream idle (the verifier waiting for its
last peer); then the wall clock around the calls, from the start of the last
arrival to the verdict's return, the three routes alternating on the same rows:

  a  fused     bk_collect_add_noised_finish
  b  sequence  bk_collect_add_noised, then bk_collect_finish (what it replaces)
  c  host      the noise added by numpy on a host core into a pinned row, then
               bk_collect_add_finish (host noising after the fused plain
               arrival; not applicable to device rows)

collect_stats() must show the path each took, and the verdicts of a and b must
agree bitwise (c's too: the same arithmetic in the same order).  Three runs (a
child process each, under its own time limit, behind one more that only warms
the machine up and is not counted); every figure is the median of the runs'
medians with [min .. max] over the runs.  `a_below_b_every_run` is the routing
rule's test: every fused run below every sequence run.  `a_vs_c` is reported
whichever way it falls.  A library without the entry (an older commit) runs b
and c alone.  Not a pass/fail gate; prints one JSON line per run and writes the
summary.
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
REPS, RUNS, LIMIT = 30, 3, 300
FUSED = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 1}
TWO = {"border": 1, "border_reduce": 1, "one_launch_finishes": 1, "fused_arrivals": 0}


def run_once():
    """(child) every configuration once -> one JSON line"""
    import numpy as np
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    have_fused = "bk_collect_add_noised_finish" in _lib.SIGNATURES
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "fused_entry": have_fused,
           "configs": {}}
    for tag, (n, d, f) in sorted(SHAPES.items()):
        Xd = torch.empty((n, d), dtype=torch.float64, device="cuda")
        eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64, n, d, d, 0, d, 20261020, f)
        eng.synchronize()
        Xh = Xd.cpu()
        Xp = Xh.pin_memory()
        gen = torch.Generator().manual_seed(d)
        Nh = 1e-2 * torch.randn((2, d), dtype=torch.float64, generator=gen)
        Np, Nd = Nh.pin_memory(), Nh.cuda()
        torch.cuda.synchronize()
        pin_row = torch.empty(d, dtype=torch.float64).pin_memory()  # route c's noised row
        tmp = np.empty(d)
        m = n - f
        sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
        sc, mean = np.empty(n), np.empty(d)
        settings = [("pinned", Xp, Np, _lib.BK_HOST_PINNED, 1), ("pinned", Xp, Np, _lib.BK_HOST_PINNED, 2),
                    ("pageable", Xh, Nh, _lib.BK_HOST, 1), ("pageable", Xh, Nh, _lib.BK_HOST, 2),
                    ("device", Xd, Nd, _lib.BK_DEVICE, 1)]
        for src, X, N, where, k in settings:
            base = X.data_ptr()

            def rows(i, cnt=1):
                return (ctypes.c_void_p * cnt)(*[base + (i + q) * d * 8 for q in range(cnt)])

            def resident():
                eng.collect_begin(n, d, np.float64)
                for i in range(0, n - 1, 8):
                    cnt = min(8, n - 1 - i)
                    eng.collect_add_ptr(rows(i, cnt), cnt, where)
                eng.synchronize()
                return eng.collect_stats()

            last = rows(n - 1)
            nz = (ctypes.c_void_p * k)(*[N.data_ptr() + q * d * 8 for q in range(k)])
            host = where != _lib.BK_DEVICE
            if host:
                dv = X[n - 1].numpy()
                nv = [N[q].numpy() for q in range(k)]
                pv = pin_row.numpy()
            args = (None, n, f, None, sel.ctypes.data, ctypes.addressof(mo), sc.ctypes.data,
                    mean.ctypes.data)

            def fused():
                _lib.check(L.bk_collect_add_noised_finish(eng.ctx, last[0], nz, k, where, *args))

            def sequence():
                _lib.check(L.bk_collect_add_noised(eng.ctx, last, nz, k, 1, where, None))
                _lib.check(L.bk_collect_finish(eng.ctx, None, n, f, sel.ctypes.data,
                                               ctypes.addressof(mo), sc.ctypes.data,
                                               mean.ctypes.data))

            def host_noised():
                # delta + ((0 + v_0) + .. + v_{k-1}) / k, the entry's order
                if k == 1:
                    np.add(0.0, nv[0], out=tmp)
                else:
                    np.add(nv[0], nv[1], out=tmp)
                np.divide(tmp, float(k), out=tmp)
                np.add(dv, tmp, out=pv)
                _lib.check(L.bk_collect_add_finish(eng.ctx, pin_row.data_ptr(), _lib.BK_HOST_PINNED,
                                                   *args))

            routes = []
            if have_fused:
                routes.append(("fused", fused, None))
            routes.append(("sequence", sequence, TWO))
            if host:
                routes.append(("host", host_noised, FUSED))
            ts = {name: [] for name, _, _ in routes}
            paths = {}
            got = {}
            for r in range(REPS + 3):  # the first three of each: warm-up
                for name, call, want in routes:
                    s0 = resident()
                    t0 = time.perf_counter()
                    call()
                    t1 = time.perf_counter()
                    s1 = eng.collect_stats()
                    took = {q: s1[q] - s0[q] for q in s1}
                    if want is None:  # the fused entry: the launch, or the two calls inside it
                        assert took in (FUSED, TWO), (name, took)
                        paths[name] = "fused" if took == FUSED else "sequence"
                    else:
                        assert took == want, (name, took)
                    got[name] = (sel.copy(), sc.copy(), mean.copy())
                    if r >= 3:
                        ts[name].append((t1 - t0) * 1e6)
                for name in got:
                    for q in range(3):
                        assert np.array_equal(got[name][q].view(np.int64),
                                              got["sequence"][q].view(np.int64)), (name, q)
            key = "%s/%s/k%d" % (tag, src, k)
            out["configs"][key] = {name: {"median_us": statistics.median(v), "min_us": min(v)}
                                   for name, v in ts.items()}
            out["configs"][key]["fused_entry_path"] = paths.get("fused")
        del Xp, Np
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(child) one run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18",
                                                  "collect_arrive_noised_bench.json"))
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
        for name in ("fused", "sequence", "host"):
            if name not in runs[0]["configs"][key]:
                continue
            meds = [r["configs"][key][name]["median_us"] for r in runs]
            rec[name + "_us"] = {"median": statistics.median(meds), "min": min(meds),
                                 "max": max(meds)}
        if "fused_us" in rec:
            fu, sq = rec["fused_us"], rec["sequence_us"]
            rec["a_minus_b_us"] = fu["median"] - sq["median"]
            rec["a_below_b_every_run"] = bool(fu["max"] < sq["min"])
            if "host_us" in rec:
                rec["a_minus_c_us"] = fu["median"] - rec["host_us"]["median"]
                rec["a_vs_c"] = ("ahead" if fu["max"] < rec["host_us"]["min"] else
                                 "behind" if fu["min"] > rec["host_us"]["max"] else "level")
            rec["fused_entry_path"] = runs[0]["configs"][key]["fused_entry_path"]
        results[key] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/collect_arrive_noised_bench.py", "runs": RUNS,
                   "reps_per_run": REPS, "device": runs[0]["device"],
                   "fused_entry": runs[0]["fused_entry"], "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
