#!/usr/bin/env python3
"""Real score error of every path against the exact double-double reference, on
an MI355X: the figures behind tests/test_gpu_exact_scores.py's sharper gate.

Runs that module's cases (tests/exact_cases.py) and no others, through the
module's own run_case with the gate off, and writes per case the GPU's largest
|s - s*|, the CPU oracle's on the same inputs, e_here, their ratios and the rung
counts, then the factor K of the gate: the next power of two at or above 4x the
largest (GPU error) / max(oracle error, 4 ulp of the largest exact score) over
the exact-arithmetic cases (u_G = 2^-53, no int8 term).  The 4x is two bits of
headroom for a summation order that is legitimately not the oracle's (MFMA
4-wide k-steps, split-K partials).  A case whose e_here / max(oracle error,
4 ulp) does not exceed K gains nothing from the gate and is listed as dropped.

    python tools/exact_scores_report.py [--out profiles/r20/exact_scores.json]
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20", "exact_scores.json"))
    args = ap.parse_args()

    import torch
    import exact_cases as EC
    import test_gpu_exact_scores as T
    from biscotti_amd.krum import Engine
    from oracle import oracle as O

    O.lib()
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    cases = []
    try:
        for case in EC.CASES:
            fig = T.run_case(eng, O, case, sharp_k=None)
            fig["exact_path"] = EC.exact_path(case)
            cases.append(fig)
            print("%-34s gpu %.3e oracle %.3e e_here %.3e gpu/floor %8.2f e_here/floor %.2e  %d+%d"
                  % (fig["id"], fig["gpu_err"], fig["oracle_err"], fig["e_here"],
                     fig["err_over_floor"], fig["e_here_over_floor"], fig["unflagged"],
                     fig["flagged"]), flush=True)
    finally:
        eng.close()
    worst = max(c["err_over_floor"] for c in cases if c["exact_path"])
    K = 2.0 ** math.ceil(math.log2(4.0 * worst))
    dropped = [c["id"] for c in cases if c["exact_path"] and not K < c["e_here_over_floor"]]
    out = dict(device=torch.cuda.get_device_name(0), worst_err_over_floor=worst, K=K,
               gate_dropped=dropped, committed_K=T.SHARP_K, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("worst (GPU error) / max(oracle error, 4 ulp) = %.3f -> K = %g; gate dropped for %s"
          % (worst, K, dropped or "no case"))


if __name__ == "__main__":
    main()
