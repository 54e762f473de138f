"""The gradient step's reference-run goldens (tests/golden/grad_*.npz, made by
tests/golden/gen_grad_goldens.py) with their regenerated inputs, and the gates
the tests hold results to (test infrastructure only)."""
import functools
import hashlib
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP64_GATE = 1e-9  # the project's fp64 gate, in units of the norm-wise scale


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLD, "grad_cases.json")) as fp:
        return json.load(fp)


def names(kind):
    return sorted(n for n, p in manifest().items() if p["kind"] == kind)


@functools.lru_cache(maxsize=None)
def load(name):
    """A case: its parameters p, inputs X, y, ww, idx (None: every row), noise
    (or None) and the reference's delta, loss (and norm).  Treat as read-only."""
    import gen_grad_goldens as G
    p = manifest()[name]
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    if p["kind"] == "logistic":
        X, y, ww, _ = G.make_logistic(**p)
        ysha = _sha(y.astype(np.float64))
    else:
        X, y, ww = G.make_softmax(**p)
        ysha = _sha(y)
    assert _sha(X) == z["X_sha256"].tobytes(), name
    assert ysha == z["y_sha256"].tobytes(), name
    assert _sha(ww) == z["ww_sha256"].tobytes(), name
    idx = z["idx"] if len(z["idx"]) else None
    return dict(p=p, X=X, y=y, ww=ww, idx=idx, noise=z["noise"] if "noise" in z else None,
                delta=z["delta"], loss=float(z["loss"]),
                norm=float(z["norm"]) if "norm" in z else None)


def softmax_gate(din, count):
    """The golden is torch fp32: the forward bound of an fp32 dot of length d_in
    followed by a sum of length count, in units of the scale."""
    return (din + count + 8) * 2.0 ** -24
