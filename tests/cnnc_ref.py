"""The one-layer cifar CNN's arithmetic (include/bk.h, bk_cnnc_shape) in plain
numpy fp64: the reference of tests/test_gpu_cnnc.py and of the torch goldens.
near_ties, counts and U are cnn_ref's: the rule is the same."""
import numpy as np

from cnn_ref import U, counts, near_ties  # noqa: F401

CIFAR = (3, 32, 32, 3, 3, 20, 10)


def dims(shape):
    ci, h, w, k, pad, co, C = shape
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    F = co * oh * ow
    return oh, ow, F, co * ci * k * k + co + C * F + C


def gammas(shape):
    T, F = shape[0] * shape[3] * shape[3], dims(shape)[2]
    gam = lambda n: n * U / (1.0 - n * U)
    g = gam(float(F + 1))
    return g * (1.0 + 2.0 ** -10), (gam(float(T + 1)) + 1.001 * U) * (1.0 + g) * (1.0 + 2.0 ** -20)


def make_case(shape, nv, seed):
    """A torch-default model (uniform in +-1/sqrt(fan_in)), images uniform in
    [-1, 1] and random labels: (ww float64, X float32 nv x (c_in h w), y int32)."""
    ci, h, w, k, pad, co, C = shape
    F, d = dims(shape)[2:]
    rng = np.random.default_rng(seed)
    ww = np.empty(d)
    nc = co * ci * k * k + co
    ww[:nc] = rng.uniform(-1, 1, nc) / np.sqrt(ci * k * k)
    ww[nc:] = rng.uniform(-1, 1, d - nc) / np.sqrt(F)
    X = rng.uniform(-1, 1, (nv, ci * h * w)).astype(np.float32)
    return ww, X, rng.integers(0, C, nv).astype(np.int32)


def forward(shape, ww, X):
    """(fp32 logits, the bound E) of every sample, both nv x C."""
    ci, h, w, k, pad, co, C = shape
    oh, ow, F, d = dims(shape)
    gF, ge = gammas(shape)
    nv, T = X.shape[0], ci * k * k
    w32 = np.asarray(ww, dtype=np.float64).astype(np.float32).astype(np.float64)
    cw, cb = w32[:co * T].reshape(co, ci, k, k), w32[co * T:co * T + co]
    fw, fb = w32[co * T + co:d - C].reshape(C, F), w32[d - C:]
    xp = np.zeros((nv, ci, h + 2 * pad, w + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + w] = X.reshape(nv, ci, h, w)
    acc, mag = np.zeros((nv, co, oh, ow)), np.zeros((nv, co, oh, ow))
    with np.errstate(all="ignore"):
        for c in range(ci):
            for ky in range(k):
                for kx in range(k):
                    patch, tap = xp[:, None, c, ky:ky + oh, kx:kx + ow], cw[None, :, c, ky, kx, None, None]
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


def predict(shape, ww, X):
    """(argmax as numpy's: the first maximum, NaN wins; near-tie flags)."""
    lg, E = forward(shape, ww, X)
    return np.argmax(lg, axis=1), near_ties(lg, E)


def roni(shape, ww, deltas, X, y, idx):
    """bk_roni_cnnc_batches: (scores n, near ties n x 2); idx is n x 2 x nb."""
    scores, near = np.empty(len(deltas)), np.empty((len(deltas), 2), dtype=np.int32)
    for j, delta in enumerate(deltas):
        err = [0.0, 0.0]
        for e, model in enumerate((ww, ww + delta)):
            rows = idx[j, e]
            err[e], _, near[j, e] = counts(*predict(shape, model, X[rows]), y[rows])
        scores[j] = err[1] - err[0]
    return scores, near
