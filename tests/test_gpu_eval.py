"""GPU: the convergence check (bk_eval*, bk_block_finish_eval).

  goldens   the reference's train_error / test_error and getTestErr /
            get17AttackRate on repo inputs (tests/golden/gen_eval_goldens.py)
  identity  bitwise the base-model evaluation of bk_roni / bk_roni_softmax:
            their score is err(ww + delta) - err(ww) of two bk_eval calls
  oracle    inputs of small integers and dyadic fractions, on which every
            summation order is exact: the counts are numpy's
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from biscotti_amd import _lib as L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = L.BK_HOST


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def ev(engine, ww, sets):
    err, wrong, near = engine.eval(ww, sets)
    return err.copy(), wrong.copy(), near.copy()


# ---- exact inputs and their numpy counts ---------------------------------------
def exact_logistic(seed, nv, d, ldv=None, labels=(-1.0, 1.0)):
    rng = np.random.default_rng(seed)
    buf = rng.integers(-3, 4, (nv, ldv or d)).astype(np.float64)
    X = buf[:, :d]
    w = rng.integers(-2, 3, d).astype(np.float64)
    if not w.any():
        w[0] = 1.0
    y = rng.choice(np.array(labels), nv)
    return X, y, w


def np_logistic(X, y, w):
    # every product and partial sum is a small integer: exact in any order
    return int(np.sum(np.sign(X @ w) != y))


def exact_softmax(seed, nv, din, C):
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, (nv, din)).astype(np.float32)
    W = rng.integers(-16, 17, (C, din)) / 8.0
    b = rng.integers(-8, 9, C) / 8.0
    y = rng.integers(0, C, nv).astype(np.int32)
    return X, y, np.concatenate([W.ravel(), b])


def np_softmax(X, y, ww, C):
    """(wrong, near ties): the logits are exact, so numpy's argmax (the first
    maximum, NaN wins) and include/bk.h's near-tie rule in fp64 are the kernel's."""
    import gen_eval_goldens as G
    good, near = G.softmax_counts(X, y, ww, C)
    return len(y) - good, near


# ---- goldens ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eval_credit_like", "eval_labels01"])
def test_logistic_goldens(engine, name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    engine.eval_set_logistic(0, z["X_train"], z["y_train"])
    engine.eval_set_logistic(1, z["X_test"], z["y_test"])
    err, wrong, near = ev(engine, z["ww"], [0, 1])
    print(name, err, wrong, "reference", z["err"], z["wrong"])
    assert wrong.tolist() == z["wrong"].tolist()
    assert err.tobytes() == z["err"].tobytes()
    assert near.tolist() == [0, 0]


@pytest.mark.parametrize("name", ["eval_mnist", "eval_lfw", "eval_2class"])
def test_softmax_goldens(engine, name):
    import json
    import gen_eval_goldens as G
    p = json.load(open(os.path.join(GOLD, "eval_cases.json")))[name]
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    kw = {k: p[k] for k in ("seed", "nv", "din", "C", "nv_attack", "nv_skipped") if k in p}
    test, attack, _, ww = G.make_softmax(**kw)
    assert _sha(test[0]) == z["X_test_sha256"].tobytes()
    assert _sha(attack[0]) == z["X_attack_sha256"].tobytes()
    assert _sha(ww) == z["ww_sha256"].tobytes()
    assert np.array_equal(test[1], z["y_test"]) and np.array_equal(attack[1], z["y_attack"])
    engine.eval_set_softmax(1, test[0], test[1], p["C"])
    engine.eval_set_softmax(2, attack[0], attack[1], p["C"])
    err, wrong, near = ev(engine, ww, [1, 2])
    print(name, err, wrong, near, "reference", z["err"], z["wrong"])
    assert near.tolist() == [0, 0]  # the fixtures were drawn without near ties
    assert wrong.tolist() == z["wrong"].tolist()
    assert err.tobytes() == z["err"].tobytes()


def test_model_evaluator_on_the_goldens(engine):
    from biscotti_amd.evaluate import ModelEvaluator
    z = np.load(os.path.join(GOLD, "eval_credit_like.npz"), allow_pickle=False)
    m = ModelEvaluator(train=(z["X_train"], z["y_train"]), test=(z["X_test"], z["y_test"]),
                       engine=engine)
    assert m.train_error(z["ww"]) == z["err"][0] and m.test_error(z["ww"]) == z["err"][1]
    assert m.check_convergence(z["ww"], 0.2) == (True, z["err"][0], None)
    assert m.check_convergence(z["ww"], 0.1) == (False, z["err"][0], None)
    with pytest.raises(ValueError):
        m.attack_rate(z["ww"])
    X, y, ww = exact_softmax(5, 90, 20, 4)
    Xa, ya, _ = exact_softmax(6, 33, 20, 4)
    m = ModelEvaluator(test=(X, y), attack=(Xa, ya), n_classes=4, engine=engine)
    conv, e, rate = m.check_convergence(ww, 2.0)
    assert conv is True and e == 1.0 - (90 - np_softmax(X, y, ww, 4)[0]) / 90.0
    assert rate == 1.0 - (33 - np_softmax(Xa, ya, ww, 4)[0]) / 33.0 == m.attack_rate(ww)


# ---- identity with the RONI entries, bitwise ----------------------------------------
def test_identity_with_bk_roni(engine):
    rng = np.random.default_rng(41)
    lib = L.lib()
    for nv, d in ((1000, 25), (300, 100)):
        X = rng.standard_normal((nv, d))
        y = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
        ww = rng.standard_normal(d)
        delta = 0.5 * rng.standard_normal((1, d))
        w2 = ww + delta[0]
        L.check(lib.bk_roni_set_validation(engine.ctx, X.ctypes.data, nv, d, d, y.ctypes.data))
        score = np.zeros(1)
        L.check(lib.bk_roni(engine.ctx, ww.ctypes.data, delta.ctypes.data, 1, d, d,
                            score.ctypes.data))
        engine.eval_set_logistic(3, X, y)
        e0, _, _ = ev(engine, ww, [3])
        e2, _, _ = ev(engine, w2, [3])
        assert (e2 - e0).tobytes() == score.tobytes()
        assert e0[0] != e2[0]  # the update moves the error: the score is no trivial 0


@pytest.mark.parametrize("nv,din,C", [(500, 784, 10), (130, 37, 12), (64, 5, 2)])
def test_identity_with_bk_roni_softmax(engine, nv, din, C):
    import gen_roni_softmax_goldens as R
    X, y, ww, D = R.make_case(200 + C, nv, din, C, 1, 10, n_bad=1)
    w2 = ww + D[0]
    lib = L.lib()
    L.check(lib.bk_roni_softmax_set_validation(engine.ctx, X.ctypes.data, nv, din, din,
                                               y.ctypes.data, C))
    score, near = np.zeros(1), np.zeros(2, dtype=np.int32)
    L.check(lib.bk_roni_softmax(engine.ctx, ww.ctypes.data, D.ctypes.data, 1, D.shape[1],
                                score.ctypes.data, near.ctypes.data))
    engine.eval_set_softmax(0, X, y, C)
    e0, _, n0 = ev(engine, ww, [0])
    e2, _, n2 = ev(engine, w2, [0])
    print("near ties", near, n0, n2, "errors", e0, e2)
    assert (e2 - e0).tobytes() == score.tobytes()
    assert [int(n0[0]), int(n2[0])] == near.tolist()
    assert e0[0] != e2[0]


# ---- the exact-arithmetic oracle ------------------------------------------------------
def test_logistic_oracle_zero_dots_and_nan(engine):
    X, y, w = exact_logistic(7, 333, 25, labels=(-1.0, 0.0, 1.0))
    X[:40] = 0.0                      # dots of exactly 0: sign 0 equals a label 0 only
    X[40:60, :] = np.array([1.0, -1.0] + [0.0] * 23) * 3.0
    w[0] = w[1] = 2.0                 # ... and 0 by cancellation
    assert (X @ w == 0).sum() >= 60
    engine.eval_set_logistic(0, X, y)
    err, wrong, near = ev(engine, w, [0])
    assert wrong[0] == np_logistic(X, y, w) and err[0] == wrong[0] / 333.0 and near[0] == 0
    wn = w.copy()
    wn[3] = np.nan                    # NaN never equals a label -- but 0 * NaN is NaN too
    _, wrong, _ = ev(engine, wn, [0])
    assert wrong[0] == 333
    yn = y.copy()
    yn[5] = np.nan                    # a NaN label is never matched either
    engine.eval_set_logistic(0, X, yn)
    _, wrong, _ = ev(engine, w, [0])
    assert wrong[0] == int(np.sum(np.sign(X @ w) != yn))


def test_softmax_oracle_ties_and_nan(engine):
    C, din, nv = 5, 12, 100
    X, y, ww = exact_softmax(9, nv, din, C)
    W = ww[:C * din].reshape(C, din)
    W[3] = W[1]                       # classes 1 and 3: exactly equal logits everywhere
    ww[C * din + 3] = ww[C * din + 1] = 2.0  # ... and on top for many samples
    X[:10] = 0.0                      # every logit its bias
    lg = X.astype(np.float64) @ W.T + ww[C * din:]
    top = lg.max(1)
    assert ((lg[:, 1] == top) & (lg[:, 3] == top)).sum() >= 10
    y[:5] = 1                         # the first maximum wins: 1, never 3
    y[5:10] = 3
    engine.eval_set_softmax(0, X, y, C)
    err, wrong, near = ev(engine, ww, [0])
    want, want_near = np_softmax(X, y, ww, C)
    assert wrong[0] == want and near[0] == want_near and near[0] >= 10
    assert err[0] == 1.0 - (nv - want) / float(nv)
    wn = ww.copy()
    wn[2 * din + 4] = np.nan          # class 2's logit is NaN for every sample: NaN wins
    _, wrong, near = ev(engine, wn, [0])
    assert wrong[0] == int(np.sum(y != 2)) and near[0] == nv
    wb = ww.copy()
    wb[C * din + 4] = np.nan          # a NaN bias alike, at the last class
    _, wrong, _ = ev(engine, wb, [0])
    assert wrong[0] == int(np.sum(y != 4))


@pytest.mark.parametrize("d", [1, 25, 32, 33, 100])
def test_logistic_shapes(engine, d):
    for i, nv in enumerate((1, 15, 16, 17, 255, 257, 1000)):
        X, y, w = exact_logistic(1000 * d + nv, nv, d, ldv=d + 3)
        assert X.strides[0] == 8 * (d + 3)
        engine.eval_set_logistic(i % 4, X, y)
        err, wrong, _ = ev(engine, w, [i % 4])
        assert wrong[0] == np_logistic(X, y, w), (nv, d)
        assert err[0] == wrong[0] / float(nv)


@pytest.mark.parametrize("C", [2, 10, 12, 16])
def test_softmax_shapes(engine, C):
    for din in (1, 3, 4, 5, 784):
        for i, nv in enumerate((1, 16, 17, 250)):
            X, y, ww = exact_softmax(100 * C + 7 * din + nv, nv, din, C)
            engine.eval_set_softmax(i, X, y, C)
            err, wrong, near = ev(engine, ww, [i])
            want, want_near = np_softmax(X, y, ww, C)
            assert (wrong[0], near[0]) == (want, want_near), (C, din, nv)
            assert err[0] == 1.0 - (nv - want) / float(nv)


# ---- several sets, replacing and clearing, RONI untouched, where ---------------------
def test_several_sets_in_one_launch(engine):
    nvs = (700, 1, 257, 64)
    data = [exact_logistic(50 + i, nv, 40) for i, nv in enumerate(nvs)]
    w = data[0][2]
    for i, (X, y, _) in enumerate(data):
        engine.eval_set_logistic(i, X, y)
    single = [ev(engine, w, [i]) for i in range(4)]
    for sets in ([2, 0], [3, 1, 0, 2], [1, 3]):
        l0, c0 = engine.eval_stats()
        err, wrong, near = ev(engine, w, sets)
        l1, c1 = engine.eval_stats()
        assert (l1 - l0, c1 - c0) == (1, 1)  # one launch whatever the number of sets
        for k, s in enumerate(sets):
            assert wrong[k] == single[s][1][0] == np_logistic(data[s][0], data[s][1], w)
            assert err[k] == single[s][0][0]
    # softmax: the model's preparation is folded into the one launch
    sm = [exact_softmax(60 + i, nv, 30, 7) for i, nv in enumerate((65, 200))]
    for i, (X, y, _) in enumerate(sm):
        engine.eval_set_softmax(i, X, y, 7)
    l0, c0 = engine.eval_stats()
    err, wrong, near = ev(engine, sm[0][2], [1, 0])
    assert [a - b for a, b in zip(engine.eval_stats(), (l0, c0))] == [1, 1]
    for k, s in enumerate((1, 0)):
        assert (wrong[k], near[k]) == np_softmax(sm[s][0], sm[s][1], sm[0][2], 7)
    # mixed kinds, another d, a set named twice: refused, the set named
    for sets, d, word in (([0, 2], 7 * 31, "set 2"), ([2], 41, "set 2"), ([2, 3, 2], 40, "set 2")):
        with pytest.raises(ValueError, match=word):
            engine.eval(np.zeros(d), sets)


def test_replace_and_clear(engine):
    X, y, w = exact_logistic(70, 100, 10)
    X2, y2, _ = exact_logistic(71, 37, 10)
    engine.eval_set_logistic(1, X, y)
    assert ev(engine, w, [1])[1][0] == np_logistic(X, y, w)
    engine.eval_set_logistic(1, X2, y2)
    err, wrong, _ = ev(engine, w, [1])
    assert wrong[0] == np_logistic(X2, y2, w) and err[0] == wrong[0] / 37.0
    engine.eval_clear(1)
    with pytest.raises(ValueError, match="set 1 is empty"):
        engine.eval(w, [1])
    engine.eval_clear(1)  # clearing an empty slot is no error
    engine.eval_set_logistic(1, X, y)
    assert ev(engine, w, [1])[1][0] == np_logistic(X, y, w)


def test_roni_state_is_untouched(engine):
    rng = np.random.default_rng(80)
    nv, d = 600, 25
    X = rng.standard_normal((nv, d))
    y = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
    ww = rng.standard_normal(d)
    delta = 0.7 * rng.standard_normal(d)
    lib = L.lib()
    L.check(lib.bk_roni_set_validation(engine.ctx, X.ctypes.data, nv, d, d, y.ctypes.data))
    L.check(lib.bk_roni_round_begin(engine.ctx, ww.ctypes.data, d, H))
    rows = (ctypes.c_void_p * 1)(delta.ctypes.data)

    def score():
        s = np.zeros(1)
        L.check(lib.bk_roni_round_score(engine.ctx, rows, 1, H, s.ctypes.data))
        return s.tobytes()

    before = score()
    Xe, ye, we = exact_logistic(81, 300, d)
    engine.eval_set_logistic(0, Xe, ye)
    engine.eval_set_logistic(2, X[:50], y[:50])
    ev(engine, we, [0, 2])
    engine.eval_clear(0)
    Xs, ys, ws = exact_softmax(82, 40, 8, 3)
    engine.eval_set_softmax(0, Xs, ys, 3)
    ev(engine, ws, [0])
    assert score() == before  # the live round and its validation set
    s = np.zeros(1)
    L.check(lib.bk_roni(engine.ctx, ww.ctypes.data, delta.ctypes.data, 1, d, d, s.ctypes.data))
    assert s.tobytes() == before


def test_where_host_pinned_device(engine):
    import torch
    X, y, w = exact_logistic(90, 500, 33)
    Xs, ys, ws = exact_softmax(91, 100, 50, 10)
    engine.eval_set_logistic(0, X, y)
    engine.eval_set_softmax(1, Xs, ys, 10)
    for model, s in ((w, 0), (ws, 1)):
        want = ev(engine, model, [s])
        pinned = torch.from_numpy(model.copy()).pin_memory()
        dev = torch.from_numpy(model).cuda()
        torch.cuda.synchronize()
        for ptr, where in ((pinned.data_ptr(), L.BK_HOST_PINNED), (dev.data_ptr(), L.BK_DEVICE)):
            sets = np.array([s], dtype=np.intc)
            err, wrong, near = np.empty(1), np.empty(1, np.int64), np.empty(1, np.int32)
            engine.eval_ptr(ptr, len(model), where, sets, err, wrong, near)
            assert (err.tobytes(), wrong[0], near[0]) == (want[0].tobytes(), want[1][0], want[2][0])


# ---- bk_block_finish_eval ----------------------------------------------------------------
def _block_case(n, d, seed, softmax):
    rng = np.random.default_rng(seed)
    g0 = rng.standard_normal(d)
    rows = [0.1 * rng.standard_normal(d) for _ in range(n)]
    acc = rng.random(n) < 0.8
    acc[0] = True
    if softmax:
        X, y, _ = exact_softmax(seed + 1, 150, 784, 10)
        Xa, ya, _ = exact_softmax(seed + 2, 70, 784, 10)
    else:
        X, y, _ = exact_logistic(seed + 1, 300, d)
        Xa, ya, _ = exact_logistic(seed + 2, 90, d)
    return g0, rows, acc, (X, y), (Xa, ya)


def _run_block(eng, n, d, softmax):
    g0, rows, acc, s1, s2 = _block_case(n, d, 300 + n, softmax)
    for slot, (X, y) in ((0, s1), (2, s2)):
        if softmax:
            eng.eval_set_softmax(slot, X, y, 10)
        else:
            eng.eval_set_logistic(slot, X, y)
    eng.eval_clear(1)
    eng.block_begin(g0, precision=4)
    eng.block_add(rows[:-1], acc[:-1])
    # the two-call sequence
    g, q, qf = eng.block_finish(want_qsum=True)
    err, wrong, near = ev(eng, g, [2, 0])
    # the one call: every output bitwise
    g2, q2, qf2, err2, wrong2, near2 = eng.block_finish_eval([2, 0], want_qsum=True)
    for a, b in ((g, g2), (q, q2), (qf, qf2), (err, err2), (wrong, wrong2), (near, near2)):
        assert a.tobytes() == b.tobytes()
    want = g0.copy()
    for r, a in zip(rows[:-1], acc[:-1]):
        if a:
            want += r
    assert g2.tobytes() == want.tobytes()
    # a refused call (a set of another d; an empty slot) leaves the block usable
    Xo, yo, _ = exact_logistic(1, 20, 3)
    eng.eval_set_logistic(3, Xo, yo)
    for sets in ([3], [1], [0, 0]):
        with pytest.raises(ValueError):
            eng.block_finish_eval(sets)
    assert eng.block_finish().tobytes() == want.tobytes()
    # a later call of the family sees the same state
    eng.block_add([rows[-1]], [1])
    want += rows[-1]
    out = eng.block_finish_eval([0])
    assert out[0].tobytes() == want.tobytes()
    assert out[1].tobytes() == ev(eng, want, [0])[0].tobytes()
    assert eng.block_count() == (n, int(acc[:-1].sum()) + 1)


@pytest.mark.parametrize("n,d,softmax", [(5, 25, False), (35, 7850, True), (6, 1000, False)])
def test_block_finish_eval(engine, n, d, softmax):
    _run_block(engine, n, d, softmax)


@pytest.mark.parametrize("seq", ["0", "1"])
def test_block_finish_eval_routes(monkeypatch, seq):
    """BK_BLOCK_EVAL_SEQ=1: the finish, then the evaluation, inside the entry;
    =0: one wait for both, at every shape.  The same bits as the routed entry."""
    from biscotti_amd.krum import Engine
    monkeypatch.setenv("BK_BLOCK_EVAL_SEQ", seq)
    e = Engine(0)
    try:
        _run_block(e, 5, 25, False)
        _run_block(e, 4, 7850, True)
    finally:
        e.close()


def test_block_collector_with_an_evaluator(engine):
    from biscotti_amd.aggregate import BlockCollector
    from biscotti_amd.evaluate import ModelEvaluator
    from biscotti_amd.krum import Update
    g0, rows, acc, s1, s2 = _block_case(6, 25, 400, False)
    m = ModelEvaluator(train=s1, engine=engine)
    bc = BlockCollector(g0, engine=engine)
    for i, (r, a) in enumerate(zip(rows, acc)):
        bc.add_update(Update(SourceID=i, Iteration=0, Delta=r, Accepted=bool(a)))
    stake, stake2 = {}, {}
    g, (conv, e, rate) = bc.create_block(stake, evaluator=m, threshold=0.5)
    plain = bc.create_block(stake2)
    assert g.tobytes() == plain.tobytes() and stake == stake2
    assert e == m.train_error(plain) and conv == (e < 0.5) and rate is None
