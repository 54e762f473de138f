"""Golden vectors for the convergence check (bk_eval), produced
by the REFERENCE's own code on repo-owned inputs.

Run once in the build container (the only place /root/reference exists):

    python tests/golden/gen_eval_goldens.py

Logistic: ``train_error`` / ``test_error`` of ML/code/logistic_model_test.py
(:13-24, bound at DistSys/honest.go:221-222), whose module body loads
"credittest" and "credittrain" through ``utils.load_dataset``: each case imports
the module afresh with a stub ``utils`` that returns the case's sets (as
gen_roni_goldens.py does for the validator).

Softmax: ``Client.getTestErr`` / ``Client.get17AttackRate``
(ML/Pytorch/client.py:146-172) on the reference's ``SoftmaxModel`` after
``Client.updateModel``, reached as gen_roni_softmax_goldens.py reaches
getTrainErr.  Both walk their loader and return the error of its LAST batch, so
a fixture's set is exactly that batch: the samples the reference scored.  The
attack set holds class-1 samples only, as the reference's attack loader does.

bk_eval's softmax error may differ from torch's only by near_ties / nv
(include/bk.h, NEAR TIES).  Every softmax case is drawn with the first seed from
its base seed on whose sets have NO near tie (the rule evaluated here in numpy),
so equality with the reference is exact; the seed used is recorded.

Saved per case (.npz, numeric arrays, allow_pickle=False): the recorded errors
and wrong counts, the model ww, and per set either X and y, or (softmax sets,
too large to commit) y and the SHA-256 of X, which tests regenerate with
make_softmax (seeded numpy PCG64) and check before use.
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LOGISTIC = "/root/reference/ML/code/logistic_model_test.py"
REF_TORCH = "/root/reference/ML/Pytorch"


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---- inputs (no reference code) ----------------------------------------------
def make_logistic(seed, nv_train, nv_test, d, label01=False, zero_rows=0):
    """creditcard-shaped sets (utils.py:86-117: a bias column of ones,
    standardised features, int labels in {-1, +1}, or {0, 1}) and a model."""
    rng = np.random.default_rng(seed)
    wstar = rng.standard_normal(d)
    sets = []
    for nv in (nv_train, nv_test):
        X = np.hstack([np.ones((nv, 1)), rng.standard_normal((nv, d - 1))])
        if zero_rows:
            X[:zero_rows] = 0.0  # sign(0) = 0: equals a label 0, never a label +-1
        y = np.where(X @ wstar + 0.5 * rng.standard_normal(nv) > 0, 1, -1).astype(int)
        if label01:
            y[y == -1] = 0
        sets.append((X, y))
    ww = wstar + 0.3 * rng.standard_normal(d)
    return sets[0], sets[1], ww


def make_softmax(seed, nv, din, C, nv_attack=0, nv_skipped=0):
    """mnist-like samples (gen_roni_softmax_goldens.make_case's): the test set
    (X, y), the attack set (class-1 samples of a second draw, or None), the
    samples of the loader's earlier batch (never scored, or None) and the model."""
    import gen_roni_softmax_goldens as R
    X, y, ww, _ = R.make_case(seed, nv + nv_skipped, din, C, 1, 10)
    attack = None
    if nv_attack:
        Xa, ya, _, _ = R.make_case(seed + 500, max(4 * C * nv_attack, 64), din, C, 1, 10)
        keep = np.flatnonzero(ya == 1)[:nv_attack]
        assert len(keep) == nv_attack
        attack = (np.ascontiguousarray(Xa[keep]), np.ascontiguousarray(ya[keep]))
    skipped = (X[:nv_skipped], y[:nv_skipped]) if nv_skipped else None
    return (np.ascontiguousarray(X[nv_skipped:]), np.ascontiguousarray(y[nv_skipped:])), attack, \
        skipped, ww


def softmax_counts(X, y, ww, C):
    """(correct, near ties) by include/bk.h's rule, in numpy fp64."""
    din = X.shape[1]
    W = ww[:C * din].reshape(C, din).astype(np.float32).astype(np.float64)
    b = ww[C * din:].astype(np.float32).astype(np.float64)
    X64 = X.astype(np.float64)
    lg = (X64 @ W.T + b).astype(np.float32).astype(np.float64)
    best = np.argmax(lg, axis=1)
    xn = np.sqrt((X64 * X64).sum(1))
    wn = np.sqrt((W * W).sum(1))
    u = 2.0 ** -24
    nn = (din + 1) * u
    g = nn / (1.0 - nn) * (1.0 + 2.0 ** -10)
    rows = np.arange(len(X))
    l1 = lg[rows, best]
    rest = lg.copy()
    rest[rows, best] = -np.inf
    l2 = rest.max(1)
    ea = g * (xn * wn[best] + np.abs(b[best]))
    emax = g * (xn * wn.max() + np.abs(b).max())
    clear = l1 - l2 - u * (np.abs(l1) + np.abs(l2)) > ea + emax
    near = ~np.isfinite(lg).all(1) | ~clear
    return int((best == y).sum()), int(near.sum())


LOGISTIC_CASES = {
    # creditcard-shaped: d = 25, labels -1 / +1
    "eval_credit_like": dict(seed=101, nv_train=1000, nv_test=333, d=25),
    # labels 0 / 1, rows of zeros (their sign 0 equals the label 0)
    "eval_labels01": dict(seed=102, nv_train=500, nv_test=77, d=25, label01=True, zero_rows=30),
}
SOFTMAX_CASES = {
    "eval_mnist": dict(seed=111, nv=1000, din=784, C=10, nv_attack=100),
    "eval_lfw": dict(seed=121, nv=120, din=8742, C=12, nv_attack=16),
    # the loader has an earlier batch: only the last one is scored
    "eval_2class": dict(seed=131, nv=300, din=24, C=2, nv_attack=40, nv_skipped=50),
}


# ---- the reference ------------------------------------------------------------
def load_logistic(train, test, tag):
    stub = types.ModuleType("utils")
    sets = {"credittrain": {"X": train[0], "y": train[1]}, "credittest": {"X": test[0], "y": test[1]}}
    stub.load_dataset = lambda name: sets[name]
    sys.modules["utils"] = stub
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_logistic_model_test_%s" % tag, REF_LOGISTIC)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_torch():
    import gen_roni_softmax_goldens as R
    R.REF = REF_TORCH
    return R.load_reference()


def loader(batches):
    import torch
    return [{"image": torch.from_numpy(X), "label": torch.from_numpy(y.astype(np.int64))}
            for X, y in batches if X is not None]


def wrong_of(err, nv):
    w = int(round(err * nv))
    assert abs(err * nv - w) < 1e-6
    return w


def main():
    manifest = {}
    for name, p in LOGISTIC_CASES.items():
        train, test, ww = make_logistic(**p)
        for X, _ in (train, test):  # BLAS order cannot move a sign: no dot near 0 but the exact zeros
            dots = np.abs(X @ ww)
            assert dots[dots != 0.0].min() > 1e-9
        ref = load_logistic(train, test, name)
        e_train, e_test = float(ref.train_error(list(ww))), float(ref.test_error(list(ww)))
        out = dict(ww=ww, X_train=train[0], y_train=train[1].astype(np.float64), X_test=test[0],
                   y_test=test[1].astype(np.float64), err=np.array([e_train, e_test]),
                   wrong=np.array([wrong_of(e_train, len(train[0])), wrong_of(e_test, len(test[0]))],
                                  dtype=np.int64))
        np.savez(os.path.join(HERE, name + ".npz"), **out)
        manifest[name] = dict(p, kind="logistic", err=out["err"].tolist(), wrong=out["wrong"].tolist())
        print(name, out["err"], out["wrong"], flush=True)

    client, softmax_model = load_torch()
    for name, p in SOFTMAX_CASES.items():
        q = dict(p)
        for seed in range(p["seed"], p["seed"] + 9):  # the first draw without a near tie
            q["seed"] = seed
            test, attack, skipped, ww = make_softmax(**q)
            counts = [softmax_counts(X, y, ww, p["C"]) for X, y in (test, attack)]
            if all(nt == 0 for _, nt in counts):
                break
        else:
            raise SystemExit("%s: no seed without near ties" % name)
        c = client.Client.__new__(client.Client)
        c.model = softmax_model.SoftmaxModel(p["din"], p["C"])
        c.testloader = loader([skipped or (None, None), test])
        c.attackloader = loader([attack])
        c.updateModel(np.array(ww))
        e_test, e_attack = float(c.getTestErr()), float(c.get17AttackRate())
        wrong = np.array([wrong_of(e_test, len(test[0])), wrong_of(e_attack, len(attack[0]))],
                         dtype=np.int64)
        # the rule's own argmax agrees with torch's: there is no near tie
        assert [len(test[0]) - counts[0][0], len(attack[0]) - counts[1][0]] == wrong.tolist()
        assert set(attack[1].tolist()) == {1}
        np.savez(os.path.join(HERE, name + ".npz"), y_test=test[1], y_attack=attack[1],
                 X_test_sha256=sha(test[0]), X_attack_sha256=sha(attack[0]), ww_sha256=sha(ww),
                 err=np.array([e_test, e_attack]), wrong=wrong)
        manifest[name] = dict(q, kind="softmax", err=[e_test, e_attack], wrong=wrong.tolist())
        print(name, "seed", q["seed"], [e_test, e_attack], wrong, flush=True)
    with open(os.path.join(HERE, "eval_cases.json"), "w") as fp:
        json.dump(manifest, fp, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
