"""GPU: the one-layer CNN's forward pass (bk_eval on a CNN set,
bk_roni_cnn_batches) against tests/cnn_ref.py, the arithmetic of
include/bk.h in numpy fp64 -- equal wrong, err, scores and near-tie counts --
and against torch's own fp32 logits of the reference's MNISTCNNModel."""
import functools
import os

import numpy as np
import pytest

import cnn_ref
from biscotti_amd import _lib as L
from biscotti_amd.evaluate import TEST, ModelEvaluator
from biscotti_amd.roni import CNNRONIValidator

pytestmark = pytest.mark.gpu

SMALL = [(5, 5, 3, 2, 1, 2), (7, 6, 3, 0, 3, 16), (9, 9, 5, 4, 16, 3)]
EVAL_CASES = [(s, nv, k) for s in SMALL for nv in (1, 15, 16, 17, 65) for k in (1, 2)] + \
             [(cnn_ref.MNIST, nv, k) for nv in (1, 17) for k in (1, 2)]
RONI_SHAPE = SMALL[2]


@functools.lru_cache(maxsize=None)
def case(shape):
    """The shape's model and samples with the reference's per-sample verdicts."""
    ww, X, y = cnn_ref.make_case(shape, 17 if shape == cnn_ref.MNIST else 65, sum(shape))
    pred, flag = cnn_ref.predict(shape, ww, X)
    for a in (ww, X, y, pred, flag):
        a.setflags(write=False)
    return ww, X, y, pred, flag


def triple(err, wrong, near, i=0):
    return err[i].tobytes(), int(wrong[i]), int(near[i])


def want(c, rows):
    err, wrong, near = cnn_ref.counts(c[3][rows], c[4][rows], c[2][rows])
    return np.float64(err).tobytes(), wrong, near


@pytest.mark.parametrize("shape,nv,nsets", EVAL_CASES)
def test_eval_against_reference(engine, shape, nv, nsets):
    c = case(shape)
    rows = [slice(0, nv), slice(len(c[2]) - nv, len(c[2]))][:nsets]  # the tile edges: nv
    for slot, r in enumerate(rows):
        engine.eval_set_cnn(slot, c[1][r], c[2][r], shape)
    out = engine.eval(c[0], list(range(nsets)))
    print(shape, nv, [triple(*out, i)[1:] for i in range(nsets)])
    for slot, r in enumerate(rows):
        assert triple(*out, slot) == want(c, r)


@pytest.mark.parametrize("nb", [1, 10, 17])
@pytest.mark.parametrize("n", [1, 3])
def test_roni_batches_against_reference(engine, nb, n):
    ww, X, y = case(RONI_SHAPE)[:3]
    rng = np.random.default_rng(100 * nb + n)
    deltas = 0.05 * rng.standard_normal((n, len(ww)))
    idx = rng.integers(0, len(y), (n, 2, nb))  # drawn with repeats
    idx[0, 1, -1] = idx[0, 1, 0]
    v = CNNRONIValidator(X, y, RONI_SHAPE, engine=engine, batch_size=nb, seed=3)
    got = v.scores(ww, deltas, idx)
    scores, near = cnn_ref.roni(RONI_SHAPE, ww, deltas, X, y, idx)
    print(nb, n, got, v.last_near_ties.ravel())
    assert got.tobytes() == scores.tobytes()
    assert np.array_equal(v.last_near_ties, near)
    # a drawn batch is the shuffled loader's last one: nv % nb samples, or nb
    assert v.draw_batches(2).shape == (2, 2, len(y) % nb or nb) and v.last_idx is idx


def test_nan_weight_and_dead_activations(engine):
    """A NaN fc weight: every sample predicts its class, the call is BK_OK and
    every sample is flagged.  Images that leave every pre-activation negative:
    all activations 0, the logits are the fc biases."""
    shape = RONI_SHAPE
    ww, X, y = (a.copy() for a in case(shape)[:3])
    h, w, k, pad, co, C = shape
    F = cnn_ref.dims(shape)[2]
    nan = ww.copy()
    nan[co * k * k + co + F + 7] = np.nan  # class 1's row
    engine.eval_set_cnn(0, X, y, shape)
    out = engine.eval(nan, [0])
    assert triple(*out) == (np.float64(1.0 - float((y == 1).sum()) / 65.0).tobytes(),
                            int((y != 1).sum()), 65)
    v = CNNRONIValidator(X, y, shape, engine=engine, batch_size=10, seed=1)
    same = np.tile(np.arange(10), (1, 2, 1))  # both evaluations on one batch: the score is 0
    assert v.scores(nan, np.zeros((1, len(ww))), same).tobytes() == np.zeros(1).tobytes()
    assert v.last_near_ties.tolist() == [[10, 10]]
    dead = ww.copy()
    dead[:co * k * k] = np.abs(dead[:co * k * k])
    dead[co * k * k:co * k * k + co] = -0.5
    Xn = -np.abs(X)
    engine.eval_set_cnn(1, Xn, y, shape)
    out = engine.eval(dead, [1])
    top = int(np.argmax(dead[-C:].astype(np.float32)))
    assert int(out[1][0]) == int((y != top).sum())
    assert triple(*out) == tuple(np.float64(t).tobytes() if i == 0 else t for i, t in
                                 enumerate(cnn_ref.counts(*cnn_ref.predict(shape, dead, Xn), y)))


def test_model_places_and_block_finish_eval(engine):
    """The model at BK_HOST_PINNED and BK_DEVICE gives BK_HOST's bits, and
    bk_block_finish_eval on a CNN set the two-call sequence's."""
    import torch
    shape = SMALL[1]
    c = case(shape)
    ev = ModelEvaluator(test=(c[1], c[2]), cnn_shape=shape, engine=engine)
    assert ev.d == len(c[0]) and ev.test_error(c[0]) == cnn_ref.counts(c[3], c[4], c[2])[0]
    base = engine.eval(c[0], [TEST])
    assert triple(*base) == want(c, slice(None)) and ev.near_ties[TEST] == base[2][0]
    pinned = torch.from_numpy(c[0].copy()).pin_memory()
    dev = torch.from_numpy(c[0].copy()).cuda()
    torch.cuda.synchronize()
    for ptr, where in ((pinned.data_ptr(), L.BK_HOST_PINNED), (dev.data_ptr(), L.BK_DEVICE)):
        err, wrong, near = np.empty(1), np.empty(1, np.int64), np.empty(1, np.int32)
        engine.eval_ptr(ptr, len(c[0]), where, np.array([TEST], dtype=np.intc), err, wrong, near)
        assert triple(err, wrong, near) == triple(*base)
    rng = np.random.default_rng(5)
    rows = [0.05 * rng.standard_normal(len(c[0])) for _ in range(3)]
    engine.block_begin(c[0])
    engine.block_add(rows, [1, 0, 1])
    g = engine.block_finish()
    two = engine.eval(g, [TEST])
    one = engine.block_finish_eval([TEST])
    assert one[0].tobytes() == g.tobytes() and triple(*one[1:]) == triple(*two)
    assert triple(*two) == tuple(np.float64(t).tobytes() if i == 0 else t for i, t in
                                 enumerate(cnn_ref.counts(*cnn_ref.predict(shape, g, c[1]), c[2])))
    with pytest.raises(ValueError):  # a softmax set of the same call: mixed kinds
        engine.eval_set_softmax(0, c[1], c[2], shape[5])
        engine.eval(c[0], [TEST, 0])


def test_against_torch(engine):
    """torch's fp32 logits of the reference's MNISTCNNModel (tests/golden/
    gen_cnn_goldens.py): every sample the GPU does not flag has torch's
    prediction, and at most half are flagged."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "cnn_mnist_logits.npz"))
    ww, X, _ = cnn_ref.make_case(cnn_ref.MNIST, len(gold["pred"]), int(gold["seed"]))
    # with torch's predictions as the labels, wrong counts the disagreements
    engine.eval_set_cnn(0, X, gold["pred"], cnn_ref.MNIST)
    _, wrong, near = engine.eval(ww, [0])
    flag = np.array([engine.eval_set_cnn(1, X[i:i + 1], gold["pred"][i:i + 1], cnn_ref.MNIST) or
                     engine.eval(ww, [1])[1:] for i in range(len(X))]).reshape(len(X), 2)
    print("flagged", near[0], "of", len(X), "disagreeing", wrong[0], "golden share", float(gold["share"]))
    assert int(flag[:, 1].sum()) == near[0] and int(flag[:, 0].sum()) == wrong[0]
    assert not np.any((flag[:, 0] == 1) & (flag[:, 1] == 0))
    assert near[0] <= len(X) // 2
