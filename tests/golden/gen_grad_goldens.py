"""Golden vectors for the gradient step (bk_grad_*), produced by
the REFERENCE's own code on repo-owned inputs.

Run once in the build container (the only place /root/reference exists):

    python tests/golden/gen_grad_goldens.py

Logistic: ``privateFun`` of ML/code/logistic_model.py (:113-140), imported with
stub ``utils`` and ``emcee`` modules (emcee is only used under diffPriv13).  Its
globals X, y, this_batch_size and samples are set as ``init`` would set them;
``np.random.seed`` before the call makes the drawn ``idx`` reproducible, and it
is recorded by drawing it once more from the same seed.  ``samples`` is all
zeros (the reference's epsilon = 0) except in the noised case, where it is a
recorded array; the noise vector is the module's own ``getNoise(iteration)``.

Softmax: ``Client.getGrad`` (ML/Pytorch/client.py:38-65) on the reference's
``SoftmaxModel`` after ``Client.updateModel``, reached through
gen_roni_softmax_goldens.load_reference(), negated as client_obj.privateFun
(:73-77) does.  The trainloader is one batch, built as gen_eval_goldens.loader
builds its loaders; criterion and optimizer are Client.__init__'s.  getGrad
drops the norm clip_grad_norm returns, so the call is wrapped to record it.

Saved per case (.npz, numeric arrays, allow_pickle=False): idx (empty: every
row), delta, loss, norm (softmax), noise (if any) and the SHA-256 of X, y and
ww, which tests regenerate with make_logistic / make_softmax (seeded numpy
PCG64) and check before use.  grad_cases.json keeps each case's parameters and
the deviation of tests/grad_ref.py from the reference measured here, in units
of the case's norm-wise scale.
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LOGISTIC = "/root/reference/ML/code/logistic_model.py"
REF_TORCH = "/root/reference/ML/Pytorch"


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---- inputs (no reference code) ----------------------------------------------
def make_logistic(seed, nn, d, batch, label01=False, margin=0.0, noise=False, **_):
    """A creditcard-shaped shard (a bias column of ones, standardised features,
    labels -1 / +1 or 0 / 1), a model, and the pre-sampled noise rows (or None).
    margin: the model is scaled so that |X w| is about that large, and every
    third label is flipped."""
    rng = np.random.default_rng(seed)
    wstar = rng.standard_normal(d)
    X = np.hstack([np.ones((nn, 1)), rng.standard_normal((nn, d - 1))])
    y = np.where(X @ wstar + 0.5 * rng.standard_normal(nn) > 0, 1, -1).astype(int)
    if label01:
        y[y == -1] = 0
    ww = 0.1 * (wstar + 0.3 * rng.standard_normal(d))
    if margin:
        ww = ww * (margin / np.median(np.abs(X @ ww)))
        y[::3] = -y[::3]  # large margins on the wrong side too
    samples = 3.0 * rng.standard_normal((100, d)) if noise else None
    return X, y, ww, samples


def make_softmax(seed, nn, din, C, xscale=1.0, **_):
    """mnist-like samples (gen_roni_softmax_goldens.make_case's) and a model."""
    import gen_roni_softmax_goldens as R
    X, y, ww, _ = R.make_case(seed, nn, din, C, 1, 10)
    if xscale != 1.0:
        X = (X * np.float32(xscale)).astype(np.float32)
    return X, y, ww


# count x d; batch >= nn: the reference takes every row and still divides by batch
LOGISTIC_CASES = {
    "grad_lg_1x1": dict(seed=201, nn=1, d=1, batch=1),
    "grad_lg_credit": dict(seed=202, nn=500, d=25, batch=10),
    "grad_lg_256x25": dict(seed=203, nn=400, d=25, batch=256),
    "grad_lg_257x33": dict(seed=204, nn=400, d=33, batch=257),
    "grad_lg_700x100": dict(seed=205, nn=900, d=100, batch=700),
    "grad_lg_full600": dict(seed=206, nn=600, d=25, batch=600),
    "grad_lg_200_b500": dict(seed=207, nn=200, d=25, batch=500),
    "grad_lg_labels01": dict(seed=208, nn=300, d=25, batch=40, label01=True),
    "grad_lg_margins": dict(seed=209, nn=300, d=25, batch=64, margin=800.0),
    "grad_lg_noise": dict(seed=210, nn=500, d=25, batch=10, noise=True),
}
# count x d_in x C
SOFTMAX_CASES = {
    "grad_sm_1x1x2": dict(seed=221, nn=1, din=1, C=2, count=0),
    "grad_sm_mnist": dict(seed=222, nn=60, din=784, C=10, count=10),
    "grad_sm_7x24x2": dict(seed=223, nn=30, din=24, C=2, count=7),
    "grad_sm_16x100x16": dict(seed=224, nn=40, din=100, C=16, count=16),
    "grad_sm_257x70x3": dict(seed=225, nn=300, din=70, C=3, count=257),
    "grad_sm_lfw": dict(seed=226, nn=12, din=8742, C=12, count=5),
    # features scaled so that the gradient's norm exceeds 100: the clip acts
    "grad_sm_clip": dict(seed=227, nn=30, din=24, C=2, count=7, xscale=2000.0),
}


def draw_idx(seed, nn, count):
    """count rows of nn without repeats, unsorted; count = 0: every row."""
    if not count:
        return np.zeros(0, dtype=np.int64)
    return np.random.default_rng(seed + 5000).permutation(nn)[:count].astype(np.int64)


# ---- the reference ------------------------------------------------------------
def load_logistic(tag):
    stub = types.ModuleType("utils")
    stub.load_dataset = lambda name: None
    sys.modules["utils"] = stub
    sys.modules["emcee"] = types.ModuleType("emcee")
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_logistic_model_%s" % tag, REF_LOGISTIC)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import grad_ref
    manifest = {}
    for name, p in LOGISTIC_CASES.items():
        X, y, ww, samples = make_logistic(**p)
        nn, d, bs = p["nn"], p["d"], p["batch"]
        mod = load_logistic(name)
        mod.X, mod.y, mod.d, mod.this_batch_size = X, y, d, bs
        mod.samples = samples if samples is not None else np.zeros((mod.expected_iters, d))
        noise = mod.getNoise(mod.iteration) if samples is not None else None
        if 0 < bs < nn:  # privateFun's own draw, repeated from the same seed
            np.random.seed(p["seed"])
            idx = np.random.choice(nn, bs, replace=False).astype(np.int64)
        else:
            idx = np.zeros(0, dtype=np.int64)
        np.random.seed(p["seed"])
        delta = np.asarray(mod.privateFun(list(ww)), dtype=np.float64)
        rows = idx if len(idx) else np.arange(nn)
        loss = float(mod.funObj(ww, X[rows, :], y[rows], bs)[0])
        mine, myloss = grad_ref.logistic(X, y, ww, idx if len(idx) else None, bs, mod.alpha,
                                         mod.lammy, noise)
        scale = grad_ref.logistic_scale(X, ww, idx if len(idx) else None, bs, mod.alpha, mod.lammy,
                                        noise)
        dev = float(np.max(np.abs(mine - delta)) / scale)
        assert np.isfinite(delta).all() and dev <= 1e-9, (name, dev)
        out = dict(idx=idx, delta=delta, loss=np.array(loss), X_sha256=sha(X),
                   y_sha256=sha(y.astype(np.float64)), ww_sha256=sha(ww))
        if noise is not None:
            out["noise"] = noise
        np.savez(os.path.join(HERE, name + ".npz"), **out)
        manifest[name] = dict(p, kind="logistic", count=int(len(rows)), alpha=mod.alpha,
                              lammy=mod.lammy, scale=scale, ref_deviation=dev,
                              loss_deviation=abs(myloss - loss) / max(abs(loss), 1.0))
        print(name, "count", len(rows), "deviation", dev, flush=True)

    import torch
    import gen_roni_softmax_goldens as R
    import gen_eval_goldens as E
    R.REF = REF_TORCH
    client, softmax_model = R.load_reference()
    nn_mod = client.nn
    recorded = []
    clip = nn_mod.utils.clip_grad_norm

    def recording_clip(*args, **kw):
        v = clip(*args, **kw)
        recorded.append(float(v))
        return v

    nn_mod.utils.clip_grad_norm = recording_clip
    for name, p in SOFTMAX_CASES.items():
        X, y, ww = make_softmax(**p)
        nn, din, C = p["nn"], p["din"], p["C"]
        idx = draw_idx(p["seed"], nn, p["count"])
        rows = idx if len(idx) else np.arange(nn)
        c = client.Client.__new__(client.Client)
        c.model = softmax_model.SoftmaxModel(din, C)
        c.criterion = nn_mod.CrossEntropyLoss()
        c.optimizer = client.optim.SGD(c.model.parameters(), lr=0.001, momentum=0.75,
                                       weight_decay=0.001)
        c.loss = 0.0
        c.trainloader = E.loader([(np.ascontiguousarray(X[rows]), y[rows])])
        c.updateModel(np.array(ww))
        del recorded[:]
        delta = (-1) * np.asarray(c.getGrad(), dtype=np.float64)
        norm, loss = recorded[-1], float(c.getLoss())
        if "xscale" in p:
            assert norm > 100.0, (name, norm)
        mine, myloss, mynorm = grad_ref.softmax(X, y, ww, idx if len(idx) else None, C)
        scale = grad_ref.softmax_scale(X, idx if len(idx) else None)
        dev = float(np.max(np.abs(mine - delta)) / scale)
        bound = (din + len(rows) + 8) * 2.0 ** -24
        np.savez(os.path.join(HERE, name + ".npz"), idx=idx, delta=delta, loss=np.array(loss),
                 norm=np.array(norm), X_sha256=sha(X), y_sha256=sha(y), ww_sha256=sha(ww))
        manifest[name] = dict(p, kind="softmax", count=int(len(rows)), scale=scale, norm=norm,
                              ref_deviation=dev, bound=bound,
                              norm_deviation=abs(mynorm - norm) / norm,
                              loss_deviation=abs(myloss - loss) / max(abs(loss), 1.0))
        print(name, "count", len(rows), "norm", norm, "deviation", dev, "bound", bound, flush=True)
    with open(os.path.join(HERE, "grad_cases.json"), "w") as fp:
        json.dump(manifest, fp, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
