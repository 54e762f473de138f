"""The one-layer cifar CNN on the GPU (bk_eval on a CNNC set, bk_roni_cnnc_batches;
DESIGN.md §5ae) against torch on this machine's CPU, 16 threads, running the same
model restated here.  Median [min..max] of three runs in one process, after one
warm-up call each.  The CPU side leaves out the reference's go-python marshalling
of the model and the scores.  eval_4096 is one 16-sample tile per compute unit:
its time is the tile's.  Writes profiles/r35/cnnc_bench.json.

    python tools/cnnc_bench.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as Fn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from biscotti_amd.krum import Engine, cnnc_model_length  # noqa: E402
from biscotti_amd.roni import CNNCRONIValidator  # noqa: E402

SHAPE = (3, 32, 32, 3, 3, 20, 10)
D = cnnc_model_length(SHAPE)
CUTS = np.cumsum([540, 20, 259200])
SHAPES = ((20, 3, 3, 3), (20,), (10, 25920), (10,))


def timed(fn):
    fn()
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts)}


def cpu_err(ww, X, y):
    """CIFARCNNModel's forward pass on the flat model, fp32."""
    cw, cb, fw, fb = (torch.from_numpy(a.reshape(s)).float() for a, s in zip(np.split(ww, CUTS), SHAPES))
    with torch.no_grad():
        x = torch.relu(Fn.conv2d(torch.from_numpy(X.reshape(-1, 3, 32, 32)), cw, cb, 1, 3))
        pred = Fn.linear(x.reshape(x.size(0), -1), fw, fb).argmax(1).numpy()
    return 1.0 - float((pred == y).mean())


def main():
    torch.set_num_threads(16)
    rng = np.random.default_rng(35)
    fan = np.concatenate([np.full(560, 27.0), np.full(259210, 25920.0)])
    ww = rng.uniform(-1, 1, D) / np.sqrt(fan)
    Xt = rng.uniform(0, 1, (10000, 3072)).astype(np.float32)
    yt = rng.integers(0, 10, 10000).astype(np.int32)
    eng = Engine(0)
    eng.eval_set_cnnc(1, Xt, yt, SHAPE)
    eng.eval_set_cnnc(2, Xt[:1000], yt[:1000], SHAPE)
    eng.eval_set_cnnc(3, Xt[:4096], yt[:4096], SHAPE)
    out = {"shape": SHAPE, "cpu_threads": 16,
           "note": "CPU: torch on the same machine, the model restated in the tool; "
                   "go-python marshalling left out"}
    out["eval_test_10000"] = {"gpu": timed(lambda: eng.eval(ww, [1])), "cpu": timed(lambda: cpu_err(ww, Xt, yt))}
    out["eval_test_10000_attack_1000"] = {
        "gpu": timed(lambda: eng.eval(ww, [1, 2])),
        "cpu": timed(lambda: (cpu_err(ww, Xt, yt), cpu_err(ww, Xt[:1000], yt[:1000])))}
    out["eval_4096"] = {"gpu": timed(lambda: eng.eval(ww, [3])),
                        "cpu": timed(lambda: cpu_err(ww, Xt[:4096], yt[:4096]))}
    v = CNNCRONIValidator(Xt, yt, SHAPE, engine=eng, batch_size=10, seed=1)
    for n in (1, 10, 100):
        deltas = 0.01 * rng.standard_normal((n, D))
        idx = v.draw_batches(n)

        def cpu():
            for j in range(n):
                cpu_err(ww, Xt[idx[j, 0]], yt[idx[j, 0]])
                cpu_err(ww + deltas[j], Xt[idx[j, 1]], yt[idx[j, 1]])
        out["roni_n%d_nb10" % n] = {"gpu": timed(lambda: v.scores(ww, deltas, idx)), "cpu": timed(cpu)}
    for k, r in out.items():
        if isinstance(r, dict):
            print(k, "gpu %.3f [%.3f..%.3f] ms" % tuple(r["gpu"].values()),
                  "cpu %.3f [%.3f..%.3f] ms" % tuple(r["cpu"].values()), flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r35", "cnnc_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
