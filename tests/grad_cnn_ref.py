"""The one-layer CNN's gradient step (include/bk.h, bk_grad_cnn) restated in
numpy float64: the reference of tests/test_gpu_grad_cnn.py and of the torch
goldens (test infrastructure only).  The forward keeps cnn_ref's conventions
(fp32-rounded model, the tap sums in fp64, the pre-activation rounded once to
fp32); the kernels' FMA chains are plain sums here, so the two agree to
rounding, not bit for bit.  The sums keep bk.h's grouping: segments, output
rows, tiles of `tiling(shape)` positions."""
import numpy as np

import cnn_ref

LDS = 131072


def tiling(shape):
    """bk.h's TS: positions per tile, a function of the shape alone."""
    h, w, k, pad, co, C = shape
    ow = w + 2 * pad - k + 1
    rows = k * (w + 2 * pad)
    rs = rows + ((4 - rows % 64) + 64) % 64
    ts = 16
    while ts > 1 and 4 * ts * rs + 12 * co * ow * (ts + 1) > LDS:
        ts -= 1
    return ts


def activations(shape, ww, Xb):
    """(a n x co x oh x ow float64 of fp32 values, torch-comparable fp32
    pre-activations, the padded images)."""
    h, w, k, pad, co, C = shape
    oh, ow, F, d = cnn_ref.dims(shape)
    n = Xb.shape[0]
    w32 = np.asarray(ww, dtype=np.float64).astype(np.float32).astype(np.float64)
    cw, cb = w32[:co * k * k].reshape(co, k, k), w32[co * k * k:co * k * k + co]
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad))
    xp[:, pad:pad + h, pad:pad + w] = Xb.reshape(n, h, w)
    acc = np.zeros((n, co, oh, ow))
    with np.errstate(all="ignore"):
        for ky in range(k):
            for kx in range(k):
                acc = acc + xp[:, None, ky:ky + oh, kx:kx + ow] * cw[None, :, ky, kx, None, None]
        pre = (acc + cb[None, :, None, None]).astype(np.float32)
        act = np.where(pre < 0, np.float32(0), pre)
    return act.astype(np.float64), pre, xp


def _tiles(n, ts):
    return [slice(p0, min(p0 + ts, n)) for p0 in range(0, n, ts)]


def step(shape, X, y, ww, idx=None, max_norm=100.0, noise=None):
    """(delta, loss, norm before clipping)."""
    h, w, k, pad, co, C = shape
    oh, ow, F, d = cnn_ref.dims(shape)
    X = np.asarray(X)
    assert X.dtype == np.float32
    r = np.arange(len(X)) if idx is None else np.asarray(idx, dtype=np.int64)
    Xb, yb, n = X[r].astype(np.float64), np.asarray(y)[r].astype(np.int64), len(r)
    w32 = np.asarray(ww, dtype=np.float64).astype(np.float32).astype(np.float64)
    nc = co * k * k + co
    fw, fb = w32[nc:d - C].reshape(C, co, oh, ow), w32[d - C:]
    a, _, xp = activations(shape, ww, Xb)
    with np.errstate(all="ignore"):
        seg = np.einsum("nkyx,ckyx->nkyc", a, fw)  # S[ch][y][s][c]
        lg = np.zeros((n, C))
        for yy in range(oh):
            Ry = np.zeros((n, C))
            for ch in range(co):
                Ry = Ry + seg[:, ch, yy]
            lg = lg + Ry
        lg = lg + fb
        m = lg.max(1, keepdims=True)
        e = np.exp(lg - m)
        s = e.sum(1, keepdims=True)
        R = e / s
        R[np.arange(n), yb] -= 1.0
        loss = float(np.sum(np.log(s[:, 0]) + m[:, 0] - lg[np.arange(n), yb]) / n)
        af = a.reshape(n, F)
        dA = (R @ fw.reshape(C, F)).reshape(n, co, oh, ow)
        g = np.where(a > 0, dA, np.where(np.isnan(a), a, 0.0))
        GW, gb, Gw, Gcb = None, None, None, None
        for t in _tiles(n, tiling(shape)):
            tW, tb = R[t].T @ af[t], R[t].sum(0)
            tw, tcb = np.zeros((co, k, k)), np.zeros(co)
            for yy in range(oh):  # T_y, then the chain over y
                for ky in range(k):
                    for kx in range(k):
                        tw[:, ky, kx] += np.einsum("nkx,nx->k", g[t, :, yy], xp[t, yy + ky, kx:kx + ow])
                tcb += g[t, :, yy].sum((0, 2))
            first = GW is None
            GW, gb = (tW, tb) if first else (GW + tW, gb + tb)
            Gw, Gcb = (tw, tcb) if first else (Gw + tw, Gcb + tcb)
        grad = np.concatenate([Gw.ravel(), Gcb, GW.ravel(), gb]) / float(n)
        norm = float(np.sqrt(np.sum(grad * grad)))
        coef = max_norm / (norm + 1e-6)
        if not coef >= 1:
            grad = grad * coef
        delta = -grad
        if noise is not None:
            delta = delta + np.asarray(noise, dtype=np.float64)
    return delta, loss, norm


def scale(shape, X, ww, idx=None, noise=None):
    """max(largest mean |a|, largest mean |x|, 1) [+ the largest |noise|], the
    means over the batch."""
    X = np.asarray(X)
    r = np.arange(len(X)) if idx is None else np.asarray(idx, dtype=np.int64)
    Xb = X[r].astype(np.float64)
    a = activations(shape, ww, Xb)[0]
    s = max(float(np.abs(a).mean(0).max()), float(np.abs(Xb).mean(0).max()), 1.0)
    if noise is not None:
        s += float(np.max(np.abs(noise)))
    return s


def torch_gate(shape, count):
    """The goldens are torch fp32: (chain length + 8) 2^-24 in units of the
    scale.  The longest chain behind a gradient entry runs through the fc sum
    (F), the batch (count), the conv gradient's (y, x, position) sum (oh ow TS)
    and the taps (k k)."""
    oh, ow, F, _ = cnn_ref.dims(shape)
    return (F + count + oh * ow * tiling(shape) + shape[2] ** 2 + 8) * 2.0 ** -24


def golden_names():
    return sorted(_manifest())


def _manifest():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_cnn_cases.json")) as fp:
        return json.load(fp)


def load_golden(name):
    """A torch golden (tests/golden/gen_grad_cnn_goldens.py) with its inputs
    rebuilt from the seed and checked against the recorded hashes."""
    import hashlib
    import os
    p = _manifest()[name]
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    ww, X, y = cnn_ref.make_case(cnn_ref.MNIST, p["nn"], p["seed"])
    ww = ww * p["wscale"]
    for a, key in ((X, "X_sha256"), (y, "y_sha256"), (ww, "ww_sha256")):
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest() == z[key].tobytes(), name
    return dict(p=p, X=X, y=y, ww=ww, idx=z["idx"], delta=z["delta"].astype(np.float64),
                loss=float(z["loss"]), norm=float(z["norm"]))
