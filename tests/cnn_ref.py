"""The one-layer CNN's arithmetic (include/bk.h, bk_cnn_shape) in plain numpy
fp64: the reference of tests/test_gpu_cnn.py and of the torch goldens.

A product of two fp32 values is exact in fp64, so `acc + x * w` rounds once,
like the FMA chain it restates."""
import numpy as np

U = 2.0 ** -24
MNIST = (28, 28, 5, 4, 16, 10)


def dims(shape):
    h, w, k, pad, co, C = shape
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    F = co * oh * ow
    return oh, ow, F, co * k * k + co + C * F + C


def gammas(shape):
    k = shape[2]
    F = dims(shape)[2]
    gam = lambda n: n * U / (1.0 - n * U)
    g = gam(float(F + 1))
    return g * (1.0 + 2.0 ** -10), (gam(float(k * k + 1)) + 1.001 * U) * (1.0 + g) * (1.0 + 2.0 ** -20)


def make_case(shape, nv, seed):
    """A torch-default model (uniform in +-1/sqrt(fan_in)), images uniform in
    [-1, 1] and random labels: (ww float64, X float32 nv x (h w), y int32)."""
    h, w, k, pad, co, C = shape
    F, d = dims(shape)[2:]
    rng = np.random.default_rng(seed)
    ww = np.empty(d)
    nc = co * k * k + co
    ww[:nc] = rng.uniform(-1, 1, nc) / np.sqrt(k * k)
    ww[nc:] = rng.uniform(-1, 1, d - nc) / np.sqrt(F)
    X = rng.uniform(-1, 1, (nv, h * w)).astype(np.float32)
    return ww, X, rng.integers(0, C, nv).astype(np.int32)


def forward(shape, ww, X):
    """(fp32 logits, the bound E) of every sample, both nv x C."""
    h, w, k, pad, co, C = shape
    oh, ow, F, d = dims(shape)
    gF, ge = gammas(shape)
    nv = X.shape[0]
    w32 = np.asarray(ww, dtype=np.float64).astype(np.float32).astype(np.float64)
    cw, cb = w32[:co * k * k].reshape(co, k, k), w32[co * k * k:co * k * k + co]
    fw, fb = w32[co * k * k + co:d - C].reshape(C, F), w32[d - C:]
    xp = np.zeros((nv, h + 2 * pad, w + 2 * pad))
    xp[:, pad:pad + h, pad:pad + w] = X.reshape(nv, h, w)
    acc, mag = np.zeros((nv, co, oh, ow)), np.zeros((nv, co, oh, ow))
    with np.errstate(all="ignore"):
        for ky in range(k):
            for kx in range(k):
                patch, tap = xp[:, None, ky:ky + oh, kx:kx + ow], cw[None, :, ky, kx, None, None]
                acc = acc + patch * tap
                mag = mag + np.abs(patch) * np.abs(tap)
        bias = cb[None, :, None, None]
        pre = (acc + bias).astype(np.float32)
        act = np.where(pre < 0, np.float32(0), pre)
        t = gF * act.astype(np.float64) + ge * (mag + np.abs(bias))
        bnd = (t * (1.0 + 2.0 ** -22) + 2.0 ** -126).astype(np.float32)
        a, b = act.reshape(nv, F).astype(np.float64), bnd.reshape(nv, F).astype(np.float64)
        lg, E = np.zeros((nv, C)), np.zeros((nv, C))
        for f in range(F):
            lg = lg + a[:, f, None] * fw[None, :, f]
            E = E + b[:, f, None] * np.abs(fw[None, :, f])
        return (lg + fb).astype(np.float32), E + gF * np.abs(fb)


def near_ties(lg, E):
    """Per sample: could fp32 arithmetic in any order pick another class."""
    lg = lg.astype(np.float64)
    rows = np.arange(lg.shape[0])
    best = np.argmax(lg, axis=1)
    with np.errstate(all="ignore"):
        other = lg.copy()
        other[rows, best] = -np.inf
        l1, l2 = lg[rows, best], np.fmax.reduce(other, axis=1)
        emax = np.fmax.reduce(E, axis=1, initial=0.0)
        clear = l1 - l2 - U * (np.abs(l1) + np.abs(l2)) > E[rows, best] + emax
    return ~np.isfinite(lg).all(axis=1) | ~clear


def predict(shape, ww, X):
    """(argmax as numpy's: the first maximum, NaN wins; near-tie flags)."""
    lg, E = forward(shape, ww, X)
    return np.argmax(lg, axis=1), near_ties(lg, E)


def counts(pred, flag, y):
    """bk_eval's (err, wrong, near ties) of one set."""
    good = int((pred == y).sum())
    return 1.0 - float(good) / float(len(y)), len(y) - good, int(flag.sum())


def roni(shape, ww, deltas, X, y, idx):
    """bk_roni_cnn_batches: (scores n, near ties n x 2); idx is n x 2 x nb."""
    scores, near = np.empty(len(deltas)), np.empty((len(deltas), 2), dtype=np.int32)
    for j, delta in enumerate(deltas):
        err = [0.0, 0.0]
        for e, model in enumerate((ww, ww + delta)):
            rows = idx[j, e]
            err[e], _, near[j, e] = counts(*predict(shape, model, X[rows]), y[rows])
        scores[j] = err[1] - err[0]
    return scores, near
