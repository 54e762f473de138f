"""The gradient step of include/bk.h (bk_grad_logistic, bk_grad_softmax) restated
in numpy float64, tiles of 256 batch positions included (test infrastructure
only).  The kernels' FMA chains are written as plain sums here, so the
restatement agrees with the GPU to rounding, not bit for bit: tests hold the two
together at 1e-9 of the norm-wise scale below.

    logistic   funObj / privateFun, ML/code/logistic_model.py:92-140
    softmax    Client.getGrad negated, ML/Pytorch/client.py:38-65 on SoftmaxModel
    quantize   updateFloatToInt (kyber.go:698-710) with Go's int64()
"""
import numpy as np

TILE = 256
INT64_MIN = -(1 << 63)


def _rows(idx, nn):
    return np.arange(nn) if idx is None else np.asarray(idx, dtype=np.int64)


def _tile_sums(M):
    """sum over tiles of 256 rows, ascending, of each tile's column sums."""
    S = None
    for p0 in range(0, M.shape[0], TILE):
        t = np.zeros(M.shape[1])
        for row in M[p0:p0 + TILE]:
            t = t + row
        S = t if S is None else S + t
    return S


def logistic(X, y, ww, idx, batch_size, alpha=1e-2, lammy=0.01, noise=None):
    """(delta, loss)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    ww = np.asarray(ww, dtype=np.float64)
    r = _rows(idx, len(X))
    Xb, yb = X[r], y[r]
    with np.errstate(over="ignore", invalid="ignore"):
        t = yb * (Xb @ ww)
        res = -yb / (1.0 + np.exp(t))
        S = _tile_sums(Xb * res[:, None])
        g = S / float(batch_size) + lammy * ww
        delta = -alpha * g
        if noise is not None:
            delta = delta + np.asarray(noise, dtype=np.float64)
        loss = np.sum(np.logaddexp(0, -t)) + 0.5 * lammy * (ww @ ww)
    return delta, float(loss)


def logistic_scale(X, ww, idx, batch_size, alpha=1e-2, lammy=0.01, noise=None):
    """max_j [alpha (sum_i |x_ij| / batch_size + lammy |w_j|) + |noise_j|]."""
    Xb = np.abs(np.asarray(X, dtype=np.float64)[_rows(idx, len(X))])
    s = alpha * (Xb.sum(0) / float(batch_size) + lammy * np.abs(ww))
    if noise is not None:
        s = s + np.abs(noise)
    return float(np.max(s))


def softmax(X, y, ww, idx, C, max_norm=100.0, noise=None):
    """(delta, loss, norm before clipping)."""
    X = np.asarray(X)
    assert X.dtype == np.float32
    din = X.shape[1]
    ww = np.asarray(ww, dtype=np.float64)
    W = ww[:C * din].reshape(C, din).astype(np.float32).astype(np.float64)
    b = ww[C * din:].astype(np.float32).astype(np.float64)
    r = _rows(idx, len(X))
    Xb = X[r].astype(np.float64)
    yb = np.asarray(y)[r].astype(np.int64)
    n = len(r)
    with np.errstate(over="ignore", invalid="ignore"):
        lg = Xb @ W.T + b
        m = lg.max(1, keepdims=True)
        e = np.exp(lg - m)
        s = e.sum(1, keepdims=True)
        R = e / s
        R[np.arange(n), yb] -= 1.0
        G = np.empty((C, din))
        for c in range(C):
            G[c] = _tile_sums(Xb * R[:, c:c + 1])
        gb = _tile_sums(R)
        g = np.concatenate([G.ravel(), gb]) / float(n)
        norm = float(np.sqrt(np.sum(g * g)))
        coef = max_norm / (norm + 1e-6)
        if coef < 1:
            g = g * coef
        delta = -g
        if noise is not None:
            delta = delta + np.asarray(noise, dtype=np.float64)
        loss = float(np.sum(np.log(s[:, 0]) + m[:, 0] - lg[np.arange(n), yb]) / n)
    return delta, loss, norm


def softmax_scale(X, idx, noise=None):
    """max(max_k sum_i |x_ik| / count, 1) [+ max_j |noise_j|]."""
    r = _rows(idx, len(X))
    s = max(float(np.abs(np.asarray(X)[r].astype(np.float64)).sum(0).max()) / len(r), 1.0)
    if noise is not None:
        s += float(np.max(np.abs(noise)))
    return s


def quantize(delta, precision):
    """int64(delta * 10^precision) as Go on amd64 computes it."""
    scale = 1.0
    for _ in range(precision):
        scale *= 10.0
    out = np.empty(len(delta), dtype=np.int64)
    for j, v in enumerate(np.asarray(delta, dtype=np.float64) * scale):
        if v != v or v >= 9223372036854775808.0 or v < -9223372036854775808.0:
            out[j] = INT64_MIN
        else:
            out[j] = int(v)
    return out
