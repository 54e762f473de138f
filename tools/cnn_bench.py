"""The one-layer mnist CNN on the GPU (bk_eval on a CNN set, bk_roni_cnn_batches;
DESIGN.md §5y) against torch on this machine's CPU, 16 threads, running the same
model class restated here.  Median [min..max] of three runs in one process, after
one warm-up call each.  The CPU side leaves out the reference's go-python
marshalling of the model and the scores.  Writes profiles/r29/cnn_bench.json.

    python tools/cnn_bench.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from biscotti_amd.krum import Engine  # noqa: E402
from biscotti_amd.roni import CNNRONIValidator  # noqa: E402

SHAPE = (28, 28, 5, 4, 16, 10)
D = 16 * 25 + 16 + 10 * 16384 + 10


class OneLayerCNN(torch.nn.Module):
    def __init__(self, ww):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 16, 5, 1, 4)
        self.fc = torch.nn.Linear(16384, 10)
        parts = np.split(ww, [400, 416, 416 + 163840])
        with torch.no_grad():
            for p, a, shp in zip(self.parameters(), parts, ((16, 1, 5, 5), (16,), (10, 16384), (10,))):
                p.copy_(torch.from_numpy(a.reshape(shp)).float())

    def forward(self, x):
        return self.fc(torch.relu(self.conv(x)).reshape(x.size(0), -1))


def timed(fn):
    fn()
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts)}


def cpu_err(ww, X, y):
    with torch.no_grad():
        pred = OneLayerCNN(ww)(torch.from_numpy(X.reshape(-1, 1, 28, 28))).argmax(1).numpy()
    return 1.0 - float((pred == y).mean())


def main():
    torch.set_num_threads(16)
    rng = np.random.default_rng(29)
    ww = np.concatenate([rng.uniform(-0.2, 0.2, 416), rng.uniform(-1, 1, D - 416) / 128.0])
    Xt, yt = rng.uniform(-1, 1, (10000, 784)).astype(np.float32), rng.integers(0, 10, 10000).astype(np.int32)
    Xa, ya = Xt[:1000].copy(), np.full(1000, 7, np.int32)
    eng = Engine(0)
    eng.eval_set_cnn(1, Xt, yt, SHAPE)
    eng.eval_set_cnn(2, Xa, ya, SHAPE)
    out = {"shape": SHAPE, "cpu_threads": 16,
           "note": "CPU: torch on the same machine, the model class restated in the tool; "
                   "go-python marshalling left out"}
    out["eval_test_10000"] = {"gpu": timed(lambda: eng.eval(ww, [1])),
                              "cpu": timed(lambda: cpu_err(ww, Xt, yt))}
    out["eval_test_10000_attack_1000"] = {
        "gpu": timed(lambda: eng.eval(ww, [1, 2])),
        "cpu": timed(lambda: (cpu_err(ww, Xt, yt), cpu_err(ww, Xa, ya)))}
    v = CNNRONIValidator(Xt, yt, SHAPE, engine=eng, batch_size=10, seed=1)
    for n in (1, 100):
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
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r29", "cnn_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
