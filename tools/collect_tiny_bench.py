"""Measure the tiny collection (bk_set_collect_tiny, k_collect_tiny) against
today's paths at the shapes it is for.

    python tools/collect_tiny_bench.py [--out profiles/r19/collect_tiny_bench.json]
    python tools/collect_tiny_bench.py --lib <another libbk.so> --out <file>   # route (b) only

Per shape (10 x 25, 4 x 25 and 16 x 128, fp64), in ONE process on one GPU, with
every row but the last collected and the stream idle (the verifier waiting for
its last peer), the wall clock around the C calls:

  last      from the start of the last arrival's call (bk_collect_add_finish, a
            pinned row) to the verdict's return -- (a) the switch on, (b) the
            switch off (today's fused arrival), (c) bk_multikrum(BK_HOST_PINNED)
            on the packed rows, alternating
  add       the host time of one non-last bk_collect_add (the row before the
            last, a pinned row) -- (a) and (b), alternating
  noised    bk_collect_add_noised_finish with k = 1 and k = 2 from pinned,
            pageable and device rows -- (a), (b), and (c) numpy noising into a
            pinned row plus bk_collect_add_finish with the switch off

collect_tiny_stats() must show the path each route took and the verdicts of (a)
and (b) must agree bitwise.  Three runs (a child process each, under its own
time limit, behind one more that only warms the machine up and is not counted);
every figure is the median of the runs' medians with [min .. max] over the runs.
`a_below_b`: every (a) run is below every (b) run; `a_vs_c` likewise.
`routed_to_today`: the entry sends this setting to today's fused launch with
the switch on too (rows of more than 512 B: bk_collect_add_finish, and
bk_collect_add_noised_finish from device rows -- DESIGN 5p), so (a) and (b) run
the same launches; --no-cut-expected measures a build without that routing.  --lib
loads another build of the library (one without the switch: the parent's) and
measures route (b) only, to show that (b) did not move.  Not a pass/fail gate;
prints one JSON line per run and writes the summary.
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

SHAPES = {"10x25": (10, 25, 2), "4x25": (4, 25, 2), "16x128": (16, 128, 4)}  # n, d, f
REPS, RUNS, LIMIT = 30, 3, 240
TINY_SYMBOLS = ("bk_set_collect_tiny", "bk_collect_tiny_stats")


ARRIVE_MAX_BYTES = 512  # bk_collect.hip TINY_ARRIVE_MAX_BYTES


def run_once(lib_path, cut=True):
    """(child) every configuration once -> one JSON line"""
    import numpy as np
    import torch
    from biscotti_amd import _lib

    if lib_path:
        _lib.LIB_PATH = lib_path
        for s in TINY_SYMBOLS:
            _lib.SIGNATURES.pop(s, None)
    from biscotti_amd.krum import Engine

    L = _lib.lib()
    have_tiny = not lib_path
    eng = Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    PIN, HOST, DEV = _lib.BK_HOST_PINNED, _lib.BK_HOST, _lib.BK_DEVICE
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "configs": {}}

    def tiny(on):
        if have_tiny:
            eng.set_collect_tiny(on)

    def tiny_delta(t0):
        if not have_tiny:
            return None
        t1 = eng.collect_tiny_stats()
        return {k: t1[k] - t0[k] for k in t1}

    def measure(routes, prepare, check=None):
        """routes: name -> (switch, call, tiny launches expected); alternating"""
        ts = {name: [] for name in routes}
        got = {}
        for r in range(REPS + 3):  # the first three of each: warm-up
            for name, (on, call, want) in routes.items():
                tiny(on)
                prepare()
                t0s = eng.collect_tiny_stats() if have_tiny else None
                t0 = time.perf_counter()
                res = call()
                t1 = time.perf_counter()
                took = tiny_delta(t0s)
                if have_tiny:
                    assert took == want, (name, took, want)
                got[name] = res
                if r >= 3:
                    ts[name].append((t1 - t0) * 1e6)
            if check:
                check(got)
        tiny(False)
        return {name: {"median_us": statistics.median(v), "min_us": min(v)} for name, v in ts.items()}

    ZERO = {"adds": 0, "finishes": 0, "arrivals": 0}
    ARRIVAL = {"adds": 0, "finishes": 0, "arrivals": 1}
    ADD = {"adds": 1, "finishes": 0, "arrivals": 0}

    for tag, (n, d, f) in SHAPES.items():
        Xd = torch.empty((n, d), dtype=torch.float64, device="cuda")
        eng.synth_fill_ptr(Xd.data_ptr(), _lib.BK_F64, n, d, d, 0, d, 20261020, f)
        eng.synchronize()
        Xh = Xd.cpu()
        Xp = Xh.pin_memory()
        rng = np.random.default_rng(n + d)
        Nh = torch.from_numpy(1e-2 * rng.standard_normal((2, d)))
        Np, Nd = Nh.pin_memory(), Nh.cuda()
        scratch = torch.empty(d, dtype=torch.float64).pin_memory()
        m = n - f
        sel, mo = np.empty(m, np.int64), ctypes.c_int64(0)
        sc, mean = np.empty(n), np.empty(d)
        base = Xp.data_ptr()

        def rows(i, k=1):
            return (ctypes.c_void_p * k)(*[base + (i + q) * d * 8 for q in range(k)])

        def resident(upto):
            def go():
                eng.collect_begin(n, d, np.float64)
                for i in range(upto):
                    eng.collect_add_ptr(rows(i), 1, PIN)
                eng.synchronize()
            return go

        def verdict():
            return sel.copy(), sc.copy(), mean.copy()

        def same(got):
            names = [k for k in got if k in ("a", "b")]
            for k in names[1:]:
                for x, y in zip(got[names[0]], got[k]):
                    assert np.array_equal(x.view(np.int64), y.view(np.int64)), (tag, k)

        # ---- the last arrival to the verdict
        last = rows(n - 1)

        def add_finish():
            _lib.check(L.bk_collect_add_finish(eng.ctx, last[0], PIN, None, n, f, None,
                                               sel.ctypes.data, ctypes.addressof(mo),
                                               sc.ctypes.data, mean.ctypes.data))
            return verdict()

        def multikrum():
            _lib.check(L.bk_multikrum(eng.ctx, base, PIN, _lib.BK_F64, n, d, d, f, sel.ctypes.data,
                                      ctypes.addressof(mo), sc.ctypes.data, mean.ctypes.data))
            return verdict()

        long_row = cut and d * 8 > ARRIVE_MAX_BYTES
        routes = {"b": (False, add_finish, ZERO)}
        if have_tiny:
            routes = {"a": (True, add_finish, ZERO if long_row else ARRIVAL),
                      "b": (False, add_finish, ZERO), "c": (False, multikrum, ZERO)}
        out["configs"][tag + "/last"] = measure(routes, resident(n - 1), same)
        out["configs"][tag + "/last"]["routed_to_today"] = bool(long_row)

        # ---- one non-last add: the host's time
        prev = rows(n - 2)

        def add():
            _lib.check(L.bk_collect_add(eng.ctx, prev, 1, PIN, None))

        routes = {"b": (False, add, ZERO)}
        if have_tiny:
            routes = {"a": (True, add, ADD), "b": (False, add, ZERO)}
        out["configs"][tag + "/add"] = measure(routes, resident(n - 2))

        # ---- the last arrival as Delta and Noise
        for k in (1, 2):
            for src, Xs, Ns, where in (("pinned", Xp, Np, PIN), ("pageable", Xh, Nh, HOST),
                                       ("device", Xd, Nd, DEV)):
                dp = Xs.data_ptr() + (n - 1) * d * 8
                nz = (ctypes.c_void_p * k)(*[Ns.data_ptr() + j * d * 8 for j in range(k)])

                def noised_finish():
                    _lib.check(L.bk_collect_add_noised_finish(
                        eng.ctx, dp, nz, k, where, None, n, f, None, sel.ctypes.data,
                        ctypes.addressof(mo), sc.ctypes.data, mean.ctypes.data))
                    return verdict()

                dl, nv, row = Xh[n - 1].numpy(), Nh.numpy(), scratch.numpy()

                def numpy_then_add_finish():
                    # main.go:1524-1537 on the host: delta + (0 + v_0 + ..) / k
                    s = np.zeros(d)
                    for j in range(k):
                        s += nv[j]
                    np.add(dl, s / float(k), out=row)
                    _lib.check(L.bk_collect_add_finish(eng.ctx, scratch.data_ptr(), PIN, None, n, f,
                                                       None, sel.ctypes.data, ctypes.addressof(mo),
                                                       sc.ctypes.data, mean.ctypes.data))
                    return verdict()

                routes = {"b": (False, noised_finish, ZERO)}
                if have_tiny:
                    routed = long_row and where == DEV
                    routes = {"a": (True, noised_finish, ZERO if routed else ARRIVAL),
                              "b": (False, noised_finish, ZERO)}
                    if where != DEV:
                        routes["c"] = (False, numpy_then_add_finish, ZERO)
                key = "%s/noised_k%d/%s" % (tag, k, src)
                out["configs"][key] = measure(routes, resident(n - 1), same)
                out["configs"][key]["routed_to_today"] = bool(have_tiny and long_row and where == DEV)
        del Xp, Np, scratch
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(child) one run")
    ap.add_argument("--lib", default=None, help="another libbk.so: route (b) only")
    ap.add_argument("--no-cut-expected", action="store_true",
                    help="the library routes no setting to today's launches")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19",
                                                  "collect_tiny_bench.json"))
    args = ap.parse_args()
    if args.child:
        run_once(args.lib, not args.no_cut_expected)
        return 0
    runs = []
    for k in range(RUNS + 1):  # the first child warms the machine up: printed, not counted
        # a fresh child per run, under its own time limit; a failed run ends the tool
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"]
        if args.lib:
            cmd += ["--lib", os.path.abspath(args.lib)]
        if args.no_cut_expected:
            cmd += ["--no-cut-expected"]
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
        for name in ("a", "b", "c"):
            if name not in runs[0]["configs"][key]:
                continue
            meds = [r["configs"][key][name]["median_us"] for r in runs]
            rec[name + "_us"] = {"median": statistics.median(meds), "min": min(meds),
                                 "max": max(meds)}
        if "a_us" in rec:
            rec["a_below_b"] = bool(rec["a_us"]["max"] < rec["b_us"]["min"])  # every run below every run
            if "c_us" in rec:
                a, c = rec["a_us"], rec["c_us"]
                rec["a_vs_c"] = ("below" if a["max"] < c["min"] else
                                 "above" if a["min"] > c["max"] else "overlap")
        if "routed_to_today" in runs[0]["configs"][key]:
            rec["routed_to_today"] = runs[0]["configs"][key]["routed_to_today"]
        results[key] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/collect_tiny_bench.py", "runs": RUNS, "reps_per_run": REPS,
                   "device": runs[0]["device"], "library": "another build (route b only)" if args.lib
                   else "this tree", "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
