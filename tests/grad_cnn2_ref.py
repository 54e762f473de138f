"""The two-layer CNN's gradient step (include/bk.h, bk_grad_cnn2) in numpy
float64: the reference of tests/test_gpu_grad_cnn2.py, itself checked against
torch's autograd by tests/test_grad_cnn2_ref.py.  The forward is cnn2_ref's; the
backward's sums are plain numpy sums: the kernels agree to rounding, not bit for bit."""
import numpy as np

from cnn2_ref import conv, dims, pool, split


def select(a):
    """One-hot (.., 4) of each window's first maximum in (dy, dx) order; a NaN wins."""
    ph, pw = a.shape[2] // 2, a.shape[3] // 2
    win = np.stack([a[:, :, dy:2 * ph:2, dx:2 * pw:2] for dy in (0, 1) for dx in (0, 1)], axis=-1)
    return np.argmax(win, axis=-1)[..., None] == np.arange(4)


def unpool(g, sel, oh, ow):
    """g routed to the selected element of each window, zero elsewhere."""
    out = np.zeros(g.shape[:2] + (oh, ow))
    ph, pw = g.shape[2:]
    for e in range(4):
        out[:, :, e >> 1:2 * ph:2, e & 1:2 * pw:2] = np.where(sel[..., e], g, 0.0)
    return out


def maps(shape, ww, Xb):
    """fp32 pre-activations P1, P2, pooled A1, A2, the pools' selections, the fp32-rounded model."""
    ci, h, w, k, pad = shape[:5]
    model = [a.astype(np.float32).astype(np.float64) for a in split(shape, ww)]
    w1, b1, w2, b2 = model[:4]
    relu = lambda s: np.where(s < 0, np.float32(0), s)
    x = np.asarray(Xb, dtype=np.float64).reshape(len(Xb), ci, h, w)
    with np.errstate(all="ignore"):
        P1 = (conv(x, x, w1, pad)[0] + b1[None, :, None, None]).astype(np.float32)
        A1 = pool(relu(P1)).astype(np.float64)
        P2 = (conv(A1, A1, w2, pad)[0] + b2[None, :, None, None]).astype(np.float32)
        A2 = pool(relu(P2)).astype(np.float64)
    return dict(x=x, P1=P1, A1=A1, s1=select(relu(P1)), P2=P2, A2=A2, s2=select(relu(P2)), model=model)


def _wgrad(dP, src, k, pad):
    """sum over (n, oy, ox) of dP[n, co, oy, ox] srcpad[n, ci, oy + ky, ox + kx]."""
    sp = np.pad(src, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    oh, ow = dP.shape[2:]
    g = np.empty((dP.shape[1], src.shape[1], k, k))
    for ky in range(k):
        for kx in range(k):
            g[:, :, ky, kx] = np.einsum("noyx,niyx->oi", dP, sp[:, :, ky:ky + oh, kx:kx + ow])
    return g


def step(shape, X, y, ww, idx=None, max_norm=100.0, noise=None):
    """(delta, loss, norm before clipping)."""
    ci, h, w, k, pad, c1, c2, C = shape
    ph1, pw1, ph2, pw2, F, d = dims(shape)
    X = np.asarray(X)
    r = np.arange(len(X)) if idx is None else np.asarray(idx, dtype=np.int64)
    yb, n = np.asarray(y)[r].astype(np.int64), len(r)
    m = maps(shape, ww, X[r])
    w2, fw, fb = m["model"][2], m["model"][4], m["model"][5]
    with np.errstate(all="ignore"):
        a2 = m["A2"].reshape(n, F)
        lg = a2 @ fw.T + fb
        mx = lg.max(1, keepdims=True)
        e = np.exp(lg - mx)
        s = e.sum(1, keepdims=True)
        R = e / s
        R[np.arange(n), yb] -= 1.0
        loss = float(np.sum(np.log(s[:, 0]) + mx[:, 0] - lg[np.arange(n), yb]) / n)
        g2 = np.where(a2 > 0, R @ fw, np.where(np.isnan(a2), a2, 0.0)).reshape(n, c2, ph2, pw2)
        oh2, ow2 = ph1 + 2 * pad - k + 1, pw1 + 2 * pad - k + 1
        dP2 = unpool(g2, m["s2"], oh2, ow2)
        dpp = np.pad(dP2, ((0, 0), (0, 0), (k - 1, k - 1), (k - 1, k - 1)))
        dA1 = np.zeros((n, c1, ph1, pw1))
        for ky in range(k):
            for kx in range(k):
                y0, x0 = pad + k - 1 - ky, pad + k - 1 - kx
                dA1 += np.einsum("noyx,oi->niyx", dpp[:, :, y0:y0 + ph1, x0:x0 + pw1], w2[:, :, ky, kx])
        dA1 = np.where(m["A1"] > 0, dA1, np.where(np.isnan(m["A1"]), m["A1"], 0.0))
        dP1 = unpool(dA1, m["s1"], h + 2 * pad - k + 1, w + 2 * pad - k + 1)
        grad = np.concatenate([_wgrad(dP1, m["x"], k, pad).ravel(), dP1.sum((0, 2, 3)),
                               _wgrad(dP2, m["A1"], k, pad).ravel(), dP2.sum((0, 2, 3)),
                               (R.T @ a2).ravel(), R.sum(0)]) / float(n)
        norm = float(np.sqrt(np.sum(grad * grad)))
        coef = max_norm / (norm + 1e-6)
        if not coef >= 1:
            grad = grad * coef
        delta = -grad
        if noise is not None:
            delta = delta + np.asarray(noise, dtype=np.float64)
    return delta, loss, norm


def scale(shape, X, ww, idx=None, noise=None):
    """max(largest batch-mean |a1|, |a2|, |x|, 1) [+ the largest |noise|]."""
    X = np.asarray(X)
    r = np.arange(len(X)) if idx is None else np.asarray(idx, dtype=np.int64)
    m = maps(shape, ww, X[r])
    s = max(*(float(np.abs(m[key]).mean(0).max()) for key in ("A1", "A2", "x")), 1.0)
    if noise is not None:
        s += float(np.max(np.abs(noise)))
    return s


def torch_gate(shape, count):
    """(the longest chain behind an entry + 8) 2^-24 in units of the scale: the fc sum
    (F), the batch and conv1's positions (count oh1 ow1), both tap sums."""
    ci, h, w, k, pad, c1, c2, _ = shape
    oh1, ow1 = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    return (dims(shape)[4] + count * oh1 * ow1 + c2 * k * k + c1 * k * k + 8) * 2.0 ** -24
