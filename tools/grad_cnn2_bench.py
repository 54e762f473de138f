"""The two-layer lfw CNN's gradient step on the GPU (bk_grad_cnn2, DESIGN.md
§5ac) against torch on this machine's CPU, 16 threads, running the same model
restated here (autograd, clip_grad_norm_(., 100), the flatten, the quantisation
at precision 4).  Median [min..max] of three runs in one process, after one
warm-up call each.  The CPU side leaves out the reference's go-python
marshalling of the model and the gradient.  Writes profiles/r33/grad_cnn2_bench.json.

    python tools/grad_cnn2_bench.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import Engine  # noqa: E402
from cnn2_bench import CUTS, D, SHAPE, SHAPES, timed  # noqa: E402

PREC = 4


def cpu_step(ww, X, y):
    p = [torch.from_numpy(a.reshape(s)).float().requires_grad_() for a, s in zip(np.split(ww, CUTS), SHAPES)]
    x = torch.from_numpy(X.reshape(-1, 3, 62, 47))
    x = Fn.max_pool2d(torch.relu(Fn.conv2d(x, p[0], p[1], 1, 1)), 2, 2)
    x = Fn.max_pool2d(torch.relu(Fn.conv2d(x, p[2], p[3], 1, 1)), 2, 2)
    loss = Fn.cross_entropy(Fn.linear(x.reshape(x.size(0), -1), p[4], p[5]), torch.from_numpy(y.astype(np.int64)))
    loss.backward()
    torch.nn.utils.clip_grad_norm_(p, 100)
    delta = -np.concatenate([t.grad.numpy().ravel() for t in p]).astype(np.float64)
    return delta, (delta * 10.0 ** PREC).astype(np.int64)


def main():
    torch.set_num_threads(16)
    rng = np.random.default_rng(33)
    fan = np.concatenate([np.full(504, 27.0), np.full(5868, 162.0), np.full(11882, 5940.0)])
    ww = rng.uniform(-1, 1, D) / np.sqrt(fan)
    X = rng.uniform(0, 1, (2000, 3 * 62 * 47)).astype(np.float32)
    y = rng.integers(0, 2, 2000).astype(np.int32)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.grad_set_cnn2(X, y, SHAPE)
    dw = torch.from_numpy(ww).cuda()
    dout, dq = torch.empty(D, dtype=torch.float64, device="cuda"), torch.empty(D, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = {"shape": SHAPE, "d": D, "precision": PREC, "cpu_threads": 16,
           "note": "CPU: torch on the same machine, the model restated in the tool; go-python "
                   "marshalling left out.  host: model in and delta, q out through pageable memory; "
                   "device: all three stay on the device (the four launches alone)"}
    for count in (10, 256):
        idx = rng.permutation(2000)[:count].astype(np.int64)
        out["count_%d" % count] = {
            "gpu_host": timed(lambda: eng.grad_cnn2(ww, idx, precision=PREC)),
            "gpu_device": timed(lambda: eng.grad_cnn2_ptr(dw.data_ptr(), _lib.BK_DEVICE, idx, 100.0, None, PREC,
                                                          dout.data_ptr(), dq.data_ptr())),
            "cpu": timed(lambda: cpu_step(ww, X[idx], y[idx]))}
    for k, r in out.items():
        if k.startswith("count_"):
            print(k, " ".join("%s %.3f [%.3f..%.3f] ms" % ((n,) + tuple(v.values())) for n, v in r.items()),
                  flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r33", "grad_cnn2_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
