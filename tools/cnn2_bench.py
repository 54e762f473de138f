"""The two-layer lfw CNN on the GPU (bk_eval on a CNN2 set, bk_roni_cnn2_batches;
DESIGN.md §5ab) against torch on this machine's CPU, 16 threads, running the same
model restated here.  Median [min..max] of three runs in one process, after one
warm-up call each.  The CPU side leaves out the reference's go-python marshalling
of the model and the scores.  Writes profiles/r32/cnn2_bench.json.

    python tools/cnn2_bench.py [out.json]
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
from biscotti_amd.krum import Engine, cnn2_model_length  # noqa: E402
from biscotti_amd.roni import CNN2RONIValidator  # noqa: E402

SHAPE = (3, 62, 47, 3, 1, 18, 36, 2)
D = cnn2_model_length(SHAPE)
CUTS = np.cumsum([486, 18, 5832, 36, 11880])
SHAPES = ((18, 3, 3, 3), (18,), (36, 18, 3, 3), (36,), (2, 5940), (2,))


def timed(fn):
    fn()
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts)}


def cpu_err(ww, X, y):
    """LFWCNNModel's forward pass on the flat model, fp32."""
    w1, b1, w2, b2, fw, fb = (torch.from_numpy(a.reshape(s)).float() for a, s in zip(np.split(ww, CUTS), SHAPES))
    with torch.no_grad():
        x = torch.from_numpy(X.reshape(-1, 3, 62, 47))
        x = Fn.max_pool2d(torch.relu(Fn.conv2d(x, w1, b1, 1, 1)), 2, 2)
        x = Fn.max_pool2d(torch.relu(Fn.conv2d(x, w2, b2, 1, 1)), 2, 2)
        pred = Fn.linear(x.reshape(x.size(0), -1), fw, fb).argmax(1).numpy()
    return 1.0 - float((pred == y).mean())


def main():
    torch.set_num_threads(16)
    rng = np.random.default_rng(32)
    fan = np.concatenate([np.full(504, 27.0), np.full(5868, 162.0), np.full(11882, 5940.0)])
    ww = rng.uniform(-1, 1, D) / np.sqrt(fan)
    Xt = rng.uniform(0, 1, (2000, 3 * 62 * 47)).astype(np.float32)
    yt = rng.integers(0, 2, 2000).astype(np.int32)
    eng = Engine(0)
    eng.eval_set_cnn2(1, Xt, yt, SHAPE)
    out = {"shape": SHAPE, "cpu_threads": 16,
           "note": "CPU: torch on the same machine, the model restated in the tool; "
                   "go-python marshalling left out"}
    out["eval_test_2000"] = {"gpu": timed(lambda: eng.eval(ww, [1])), "cpu": timed(lambda: cpu_err(ww, Xt, yt))}
    v = CNN2RONIValidator(Xt, yt, SHAPE, engine=eng, batch_size=10, seed=1)
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
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r32", "cnn2_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
