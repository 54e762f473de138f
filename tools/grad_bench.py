#!/usr/bin/env python3
"""Per-call times of the gradient step (bk_grad_*).

    python tools/grad_bench.py [--out profiles/r26/grad_bench.json]

One process on one GPU.  Per shape: a host model (pageable in, pageable out) and
a device model (model and outputs stay on the device), each the median
[min..max] of three runs of `--reps` calls, quantisation at precision 4
included.

BASELINES, on the CPU of the same machine: a vectorised numpy restatement
(tests/grad_ref.py's arithmetic without its tile loops) and torch (fp64 for the
logistic model; an fp32 nn.Linear with CrossEntropyLoss, backward and
clip_grad_norm_ for the softmax model, as Client.getGrad runs it).  They are the
only CPU forms available here without a Go toolchain: the go-python marshalling
of oneGradientStep, which every reference call pays, is NOT in them.

A batch of more than 65,536 rows is BK_ENOTSUP: the full creditcard shard
(85,000 rows) is timed at 65,536 of its rows.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PREC = 4
# name, kind, nn, d (d_in), C, count (0: every row)
SHAPES = [
    ("creditcard_10", "logistic", 85000, 25, 0, 10),
    ("creditcard_65536", "logistic", 85000, 25, 0, 65536),
    ("mnist_10", "softmax", 6000, 784, 10, 10),
    ("mnist_256", "softmax", 6000, 784, 10, 256),
    ("lfw_10", "softmax", 400, 8742, 12, 10),
]


def timed(fn, reps):
    runs = []
    for _ in range(3):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        runs.append((time.perf_counter() - t0) / reps * 1e6)
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2),
            "max_us": round(max(runs), 2)}


def np_logistic(X, y, ww, idx, bs):
    Xb, yb = X[idx], y[idx]
    res = -yb / (1.0 + np.exp(yb * (Xb @ ww)))
    delta = -1e-2 * (Xb.T @ res / bs + 0.01 * ww)
    return delta, (delta * 1e4).astype(np.int64)


def np_softmax(X, y, ww, idx, C):
    din = X.shape[1]
    W = ww[:C * din].reshape(C, din).astype(np.float32)
    b = ww[C * din:].astype(np.float32)
    Xb, yb = X[idx], y[idx]
    lg = Xb @ W.T + b
    e = np.exp(lg - lg.max(1, keepdims=True))
    R = e / e.sum(1, keepdims=True)
    R[np.arange(len(idx)), yb] -= 1.0
    g = np.concatenate([(R.T @ Xb).ravel(), R.sum(0)]).astype(np.float64) / len(idx)
    coef = 100.0 / (np.sqrt(g @ g) + 1e-6)
    delta = -(g * coef if coef < 1 else g)
    return delta, (delta * 1e4).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    from biscotti_amd import _lib
    from biscotti_amd.krum import Engine
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    rows = []
    for name, kind, nn, d, C, count in SHAPES:
        rng = np.random.default_rng(nn + d)
        idx = rng.permutation(nn)[:count].astype(np.int64)
        reps = max(3, args.reps // (1 + count // 4096))
        if kind == "logistic":
            X = rng.standard_normal((nn, d))
            y = rng.choice([-1.0, 1.0], nn)
            ww = rng.standard_normal(d) * 0.1
            eng.grad_set_logistic(X, y)
            host = lambda: eng.grad_logistic(ww, idx, count, precision=PREC)  # noqa: E731
            ref = lambda: np_logistic(X, y, ww, idx, count)  # noqa: E731
            Xt, yt, wt = torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(ww)
            it = torch.from_numpy(idx)

            def tch():
                Xb, yb = Xt[it], yt[it]
                res = -yb / (1.0 + torch.exp(yb * (Xb @ wt)))
                delta = -1e-2 * (Xb.T @ res / count + 0.01 * wt)
                return delta, (delta * 1e4).to(torch.int64)
        else:
            X = rng.standard_normal((nn, d)).astype(np.float32)
            y = rng.integers(0, C, nn)
            ww = rng.standard_normal(C * (d + 1)) * 0.05
            eng.grad_set_softmax(X, y, C)
            host = lambda: eng.grad_softmax(ww, idx, precision=PREC)  # noqa: E731
            ref = lambda: np_softmax(X, y, ww, idx, C)  # noqa: E731
            lin = torch.nn.Linear(d, C)
            crit = torch.nn.CrossEntropyLoss()
            Xt, yt, it = torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(idx)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(ww[:C * d].reshape(C, d)).float())
                lin.bias.copy_(torch.from_numpy(ww[C * d:]).float())

            def tch():
                lin.zero_grad()
                crit(lin(Xt[it]), yt[it]).backward()
                torch.nn.utils.clip_grad_norm_(lin.parameters(), 100)
                g = np.concatenate([lin.weight.grad.numpy().ravel(), lin.bias.grad.numpy()])
                delta = -g.astype(np.float64)
                return delta, (delta * 1e4).astype(np.int64)
        dm = len(ww)
        got = host()
        want = ref()
        assert np.max(np.abs(got[0] - want[0])) <= 1e-4 * max(1.0, np.max(np.abs(want[0])))
        dw = torch.from_numpy(ww).cuda()
        dout = torch.empty(dm, dtype=torch.float64, device="cuda")
        dq = torch.empty(dm, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        loss = ctypes.c_double()
        if kind == "logistic":
            dev = lambda: eng.grad_logistic_ptr(dw.data_ptr(), _lib.BK_DEVICE, idx, count, 1e-2,  # noqa: E731
                                                0.01, None, PREC, dout.data_ptr(), dq.data_ptr(), loss)
        else:
            dev = lambda: eng.grad_softmax_ptr(dw.data_ptr(), _lib.BK_DEVICE, idx, 100.0, None,  # noqa: E731
                                               PREC, dout.data_ptr(), dq.data_ptr(), loss)
        dev()
        assert np.array_equal(dout.cpu().numpy(), got[0])
        row = {"shape": name, "kind": kind, "nn": nn, "d_in": d, "classes": C, "count": count,
               "model_entries": dm, "reps": reps, "launches_per_call": 1 if kind == "logistic" else 2,
               "gpu_host_model": timed(host, reps), "gpu_device_model": timed(dev, reps),
               "numpy": timed(ref, reps), "torch_cpu": timed(tch, reps)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/grad_bench.py", "precision": PREC, "torch_threads": torch.get_num_threads(),
           "baseline": "vectorised numpy and torch on the same host's CPU; not the reference's "
                       "go-python call, whose marshalling they leave out",
           "softmax_route": "two launches (forward, backward); the one-launch form was not built",
           "shapes": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
