"""The two-layer CNN's arithmetic and near-tie bound (include/bk.h,
bk_cnn2_shape) in plain numpy fp64: the reference of tests/test_gpu_cnn2.py and
tests/test_cnn2_ref.py.

A product of two fp32 values is exact in fp64, so `acc + x * w` rounds once,
like the FMA chain it restates."""
import numpy as np

from cnn_ref import counts, near_ties

U = 2.0 ** -24
LFW = (3, 62, 47, 3, 1, 18, 36, 2)


def dims(shape):
    """(ph1, pw1, ph2, pw2, F, d)"""
    ci, h, w, k, pad, c1, c2, C = shape
    ph1, pw1 = (h + 2 * pad - k + 1) // 2, (w + 2 * pad - k + 1) // 2
    ph2, pw2 = (ph1 + 2 * pad - k + 1) // 2, (pw1 + 2 * pad - k + 1) // 2
    F = c2 * ph2 * pw2
    return ph1, pw1, ph2, pw2, F, c1 * ci * k * k + c1 + c2 * c1 * k * k + c2 + C * F + C


def gammas(shape):
    """bk.h's (g1, g2, h2, gF, hF)"""
    ci, _, _, k, _, c1 = shape[:6]
    gam = lambda n: n * U / (1.0 - n * U)
    s, a, b, f = 1.0 + 2.0 ** -20, gam(float(ci * k * k + 1)), gam(float(c1 * k * k + 1)), \
        gam(float(dims(shape)[4] + 1))
    return (a + 1.001 * U) * s, (b + 1.001 * U) * s, (1.0 + b) * s, f * (1.0 + 2.0 ** -10), (1.0 + f) * s


def split(shape, ww):
    """The flat model's six parts as LFWCNNModel.reshape cuts them."""
    ci, _, _, k, _, c1, c2, C = shape
    F = dims(shape)[4]
    sizes = (c1 * ci * k * k, c1, c2 * c1 * k * k, c2, C * F, C)
    w1, b1, w2, b2, fw, fb = np.split(np.asarray(ww), np.cumsum(sizes)[:-1])
    return w1.reshape(c1, ci, k, k), b1, w2.reshape(c2, c1, k, k), b2, fw.reshape(C, F), fb


def make_case(shape, nv, seed):
    """A torch-default model, samples uniform in [0, 1), random labels: (ww, X, y)."""
    ci, h, w, k, _, c1, _, C = shape
    F, d = dims(shape)[4:]
    rng = np.random.default_rng(seed)
    n1, n2 = c1 * ci * k * k + c1, d - C * F - C
    fan = np.concatenate([np.full(n1, ci * k * k), np.full(n2 - n1, c1 * k * k), np.full(d - n2, F)])
    ww = rng.uniform(-1, 1, d) / np.sqrt(fan)
    return ww, rng.uniform(0, 1, (nv, ci * h * w)).astype(np.float32), rng.integers(0, C, nv).astype(np.int32)


def up32(t):
    return (t * (1.0 + 2.0 ** -22) + 2.0 ** -126).astype(np.float32)


def conv(x, e, w, pad):
    """(the chains of w . x, of |w| . e) over (ci, ky, kx) ascending, zero padding."""
    k, oh, ow = w.shape[2], x.shape[2] + 2 * pad - w.shape[2] + 1, x.shape[3] + 2 * pad - w.shape[3] + 1
    xp, ep = (np.pad(a.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad))) for a in (x, e))
    acc, bnd = np.zeros((x.shape[0], w.shape[0], oh, ow)), np.zeros((x.shape[0], w.shape[0], oh, ow))
    for ci in range(w.shape[1]):
        for ky in range(k):
            for kx in range(k):
                tap = w[None, :, ci, ky, kx, None, None]
                acc = acc + xp[:, ci, None, ky:ky + oh, kx:kx + ow] * tap
                bnd = bnd + ep[:, ci, None, ky:ky + oh, kx:kx + ow] * np.abs(tap)
    return acc, bnd


def pool(a):
    """MaxPool2d(2, 2, 0), floor mode; a NaN in the window stays."""
    ph, pw = a.shape[2] // 2, a.shape[3] // 2
    a = a[:, :, :2 * ph, :2 * pw]
    return np.maximum(np.maximum(a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2]),
                      np.maximum(a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]))


def forward(shape, ww, X):
    """(fp32 logits, the bound E) of every sample, both nv x C."""
    ci, h, w, k, pad, c1, c2, C = shape
    g1, g2, h2, gF, hF = gammas(shape)
    w1, b1, w2, b2, fw, fb = (a.astype(np.float32).astype(np.float64) for a in split(shape, ww))
    relu = lambda s: np.where(s < 0, np.float32(0), s)
    x = X.reshape(len(X), ci, h, w)
    with np.errstate(all="ignore"):
        acc, m1 = conv(x, np.abs(x), w1, pad)
        bias = b1[None, :, None, None]
        A1 = pool(relu((acc + bias).astype(np.float32)))
        q1 = up32(g2 * A1.astype(np.float64) + h2 * pool(up32(g1 * (m1 + np.abs(bias)))).astype(np.float64))
        acc, B2 = conv(A1, q1, w2, pad)
        bias = b2[None, :, None, None]
        A2 = pool(relu((acc + bias).astype(np.float32)))
        qF = up32(gF * A2.astype(np.float64) + hF * pool(up32(B2 + g2 * np.abs(bias))).astype(np.float64))
        a, q = A2.reshape(len(X), -1).astype(np.float64), qF.reshape(len(X), -1).astype(np.float64)
        lg, E = np.zeros((len(X), C)), np.zeros((len(X), C))
        for f in range(a.shape[1]):
            lg = lg + a[:, f, None] * fw[None, :, f]
            E = E + q[:, f, None] * np.abs(fw[None, :, f])
        return (lg + fb).astype(np.float32), E + gF * np.abs(fb)


def predict(shape, ww, X):
    """(argmax as numpy's: the first maximum, NaN wins; near-tie flags)."""
    lg, E = forward(shape, ww, X)
    return np.argmax(lg, axis=1), near_ties(lg, E)


def roni(shape, ww, deltas, X, y, idx):
    """bk_roni_cnn2_batches: (scores n, near ties n x 2); idx is n x 2 x nb."""
    scores, near = np.empty(len(deltas)), np.empty((len(deltas), 2), dtype=np.int32)
    for j, delta in enumerate(deltas):
        err = [0.0, 0.0]
        for e, model in enumerate((ww, ww + delta)):
            rows = idx[j, e]
            err[e], _, near[j, e] = counts(*predict(shape, model, X[rows]), y[rows])
        scores[j] = err[1] - err[0]
    return scores, near
