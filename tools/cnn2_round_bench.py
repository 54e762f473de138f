"""Measure the CNN2 verifier's round (bk_roni_cnn2_round_begin /
bk_roni_cnn2_round_score_batches) against the loop of one-update
bk_roni_cnn2_batches calls.

    python tools/cnn2_round_bench.py [--out profiles/r34/cnn2_round_bench.json] [--ns 1,10,100]

The lfw CNN verifier's iteration as deployed (Peer.VerifyUpdateRONI,
main.go:191-233): n sequential verdicts of ONE update each against one model,
on the lfw shape {3,62,47,3,1,18,36,2} with a validation set of 400 samples and
batches of 10.  In one process, per n and per kind of host rows (pageable,
pinned), two ways, alternating:
  loop   n calls of bk_roni_cnn2_batches with n = 1 (the model, the update and
         the indices go up; both evaluations run, a workgroup a whole sample)
  round  one bk_roni_cnn2_round_begin (the whole set's verdicts), then n
         bk_roni_cnn2_round_score_batches with count = 1, the band height the
         library's choice
A run times `iters` such iterations with the host clock (every score call is
synchronous; the begin's evaluation is waited for by the first score) and
reports the time per update, the begin included; each figure is the median
[min .. max] of three runs.  The round counts as ahead only where the medians
differ by more than the two min-to-max spreads together.  Also timed at n = 1:
the begin alone (with a wait behind it), and one score call alone at band
height 1, at one band, and at the library's choice, alternating.  The scores
and near-tie counts of the two ways are compared bit for bit first.
Not a pass/fail gate; prints one JSON line per case and writes them all.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from biscotti_amd import _lib  # noqa: E402

SHAPE, NV, NB, RUNS = (3, 62, 47, 3, 1, 18, 36, 2), 400, 10, 3
ITERS = {1: 200, 10: 30, 100: 4}
BANDS = {"band_1": 1, "one_band": 1 << 20, "library": 0}


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def ahead(a, b):
    """a's median below b's by more than both min-to-max spreads together"""
    return bool(b["median"] - a["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def timed(call, iters, per):
    call()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    return (time.perf_counter() - t0) * 1e6 / (iters * per)


def run_case(eng, n, ww, rng):
    import numpy as np
    import torch
    L = _lib.lib()
    d = len(ww)
    D = 0.05 * rng.standard_normal((n, d))
    idx = np.array([[rng.permutation(NV)[NV - NB:], rng.permutation(NV)[NV - NB:]]
                    for _ in range(n)], dtype=np.int64)
    iters = ITERS.get(n, 2)
    out = {"n": n, "nv": NV, "nb": NB, "d": d, "iters_per_run": iters, "runs": RUNS}
    for rows_kind in ("pageable", "pinned"):
        if rows_kind == "pageable":
            where = _lib.BK_HOST
            wbuf = ww.copy()
            rows = [D[i].copy() for i in range(n)]  # separately allocated
            wp, rp = wbuf.ctypes.data, [r.ctypes.data for r in rows]
        else:
            where = _lib.BK_HOST_PINNED
            wbuf = torch.from_numpy(ww.copy()).pin_memory()
            rows = [torch.from_numpy(D[i].copy()).pin_memory() for i in range(n)]
            wp, rp = wbuf.data_ptr(), [r.data_ptr() for r in rows]
        tabs = [(ctypes.c_void_p * 1)(p) for p in rp]
        ip = [idx[i].ctypes.data for i in range(n)]
        s_loop, s_round = np.empty(n), np.empty(n)
        n_loop, n_round = np.empty((n, 2), dtype=np.int32), np.empty((n, 2), dtype=np.int32)

        def loop():
            for i in range(n):
                _lib.check(L.bk_roni_cnn2_batches(eng.ctx, wp, rp[i], 1, d, ip[i], NB,
                                                  s_loop.ctypes.data + 8 * i,
                                                  n_loop.ctypes.data + 8 * i))

        def begin():
            _lib.check(L.bk_roni_cnn2_round_begin(eng.ctx, wp, where))

        def score(i=0):
            _lib.check(L.bk_roni_cnn2_round_score_batches(
                eng.ctx, tabs[i], 1, where, ip[i], NB, s_round.ctypes.data + 8 * i,
                n_round.ctypes.data + 8 * i))

        def rnd():
            begin()
            for i in range(n):
                score(i)

        def begin_waited():
            begin()
            _lib.check(L.bk_synchronize(eng.ctx))

        loop()
        for rows_of_band in BANDS.values():  # the same bytes at every band height
            _lib.check(L.bk_roni_cnn2_round_set_band(eng.ctx, rows_of_band))
            rnd()
            assert np.array_equal(s_loop.view(np.int64), s_round.view(np.int64)), "scores differ"
            assert np.array_equal(n_loop, n_round), "near-tie counts differ"
        per = {"loop": [], "round": [], "begin": []}
        per.update({"score_" + k: [] for k in BANDS})
        for _ in range(RUNS):
            for name, call in (("loop", loop), ("round", rnd)):  # alternating
                per[name].append(timed(call, iters, n))
            if n == 1:
                per["begin"].append(timed(begin_waited, iters, 1))
                for k, rows_of_band in BANDS.items():  # against the begin just waited for
                    _lib.check(L.bk_roni_cnn2_round_set_band(eng.ctx, rows_of_band))
                    per["score_" + k].append(timed(score, iters, 1))
        rec = {"loop_us_per_update": spread(per["loop"]),
               "round_us_per_update": spread(per["round"])}
        lo, ro = rec["loop_us_per_update"], rec["round_us_per_update"]
        rec["loop_over_round"] = lo["median"] / ro["median"]
        rec["round_ahead_beyond_spreads"] = ahead(ro, lo)
        if n == 1:
            rec["begin_alone_us"] = spread(per["begin"])
            for k in BANDS:
                rec["score_alone_us_" + k] = spread(per["score_" + k])
            rec["band_1_ahead_of_one_band_beyond_spreads"] = ahead(rec["score_alone_us_band_1"],
                                                                   rec["score_alone_us_one_band"])
        out[rows_kind] = rec
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r34", "cnn2_round_bench.json"))
    ap.add_argument("--ns", default="1,10,100", help="comma-separated updates per iteration")
    args = ap.parse_args()
    import numpy as np
    import torch
    import cnn2_ref
    from biscotti_amd.krum import Engine
    eng = Engine(0)
    ww, X, y = cnn2_ref.make_case(SHAPE, NV, 20261126)
    sh = (ctypes.c_int32 * 8)(*SHAPE)
    _lib.check(_lib.lib().bk_roni_cnn2_set_validation(eng.ctx, X.ctypes.data, NV, X.shape[1],
                                                      y.ctypes.data, sh))
    rng = np.random.default_rng(20261127)
    results = [run_case(eng, int(n), ww, rng) for n in args.ns.split(",") if n]
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/cnn2_round_bench.py", "shape": list(SHAPE),
                   "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
