"""GPU: the two-layer CNN's forward pass (bk_eval on a CNN2 set,
bk_roni_cnn2_batches) against tests/cnn2_ref.py, the arithmetic
of include/bk.h in numpy fp64: equal wrong, err, scores and near-tie counts."""
import functools

import numpy as np
import pytest

import cnn2_ref
from biscotti_amd import _lib as L
from biscotti_amd.evaluate import TEST, ModelEvaluator
from biscotti_amd.roni import CNN2RONIValidator

pytestmark = pytest.mark.gpu

SMALL = [(1, 5, 7, 3, 1, 1, 1, 2), (3, 6, 6, 3, 1, 5, 17, 3), (2, 4, 4, 1, 0, 3, 2, 16), (3, 8, 6, 2, 1, 18, 36, 2)]
EVAL_CASES = [(s, nv, k) for s in SMALL for nv in (1, 15, 16, 17, 33) for k in (1, 2)] + \
             [(cnn2_ref.LFW, nv, k) for nv in (1, 17) for k in (1, 2)]
RONI_SHAPE = SMALL[1]


@functools.lru_cache(maxsize=None)
def case(shape):
    """The shape's model and samples with the reference's per-sample verdicts."""
    ww, X, y = cnn2_ref.make_case(shape, 17 if shape == cnn2_ref.LFW else 33, sum(shape))
    pred, flag = cnn2_ref.predict(shape, ww, X)
    for a in (ww, X, y, pred, flag):
        a.setflags(write=False)
    return ww, X, y, pred, flag


def triple(err, wrong, near, i=0):
    return err[i].tobytes(), int(wrong[i]), int(near[i])


def want(shape, ww, X, y):
    err, wrong, near = cnn2_ref.counts(*cnn2_ref.predict(shape, ww, X), y)
    return np.float64(err).tobytes(), wrong, near


@pytest.mark.parametrize("shape,nv,nsets", EVAL_CASES)
def test_eval_against_reference(engine, shape, nv, nsets):
    c = case(shape)
    rows = [slice(0, nv), slice(len(c[2]) - nv, len(c[2]))][:nsets]  # the tile edges: nv
    for slot, r in enumerate(rows):
        engine.eval_set_cnn2(slot, c[1][r], c[2][r], shape)
    out = engine.eval(c[0], list(range(nsets)))
    for slot, r in enumerate(rows):
        err, wrong, near = cnn2_ref.counts(c[3][r], c[4][r], c[2][r])
        assert triple(*out, slot) == (np.float64(err).tobytes(), wrong, near)


@pytest.mark.parametrize("shape,eps", [(SMALL[1], 2.0 ** -6), (SMALL[2], 2.0 ** -13), (SMALL[3], 2.0 ** -10)])
def test_near_ties_counted(engine, shape, eps):
    """fc rows within eps of row 0, no fc bias: some samples are near ties, some not."""
    ww, X, y = (a.copy() for a in case(shape)[:3])
    F, d = cnn2_ref.dims(shape)[4:]
    C = shape[7]
    fw = ww[d - C * F - C:d - C].reshape(C, F)
    fw[1:] = fw[0] + eps * fw[1:]
    ww[d - C:] = 0.0
    ref = want(shape, ww, X, y)
    assert 0 < ref[2] < len(y)
    engine.eval_set_cnn2(0, X, y, shape)
    assert triple(*engine.eval(ww, [0])) == ref


@pytest.mark.parametrize("nb", [1, 10, 17])
@pytest.mark.parametrize("n", [1, 3])
def test_roni_batches_against_reference(engine, nb, n):
    ww, X, y = case(RONI_SHAPE)[:3]
    rng = np.random.default_rng(100 * nb + n)
    deltas = 0.05 * rng.standard_normal((n, len(ww)))
    idx = rng.integers(0, len(y), (n, 2, nb))  # drawn with repeats
    idx[0, 1, -1] = idx[0, 1, 0]
    v = CNN2RONIValidator(X, y, RONI_SHAPE, engine=engine, batch_size=nb, seed=3)
    got = v.scores(ww, deltas, idx)
    scores, near = cnn2_ref.roni(RONI_SHAPE, ww, deltas, X, y, idx)
    assert got.tobytes() == scores.tobytes()
    assert np.array_equal(v.last_near_ties, near)
    with pytest.raises(ValueError):
        v.begin_round(ww)


@pytest.mark.parametrize("part", ["conv1", "conv2", "fc", "dead"])
def test_nan_weight_and_dead_activations(engine, part):
    """One NaN weight in a layer: the call is BK_OK, the counts the restatement's.
    conv2 biases of -1e3: every activation is dead, the logits are the fc biases."""
    shape = SMALL[1]
    ww, X, y = (a.copy() for a in case(shape)[:3])
    ci, _, _, k, _, c1, c2, C = shape
    o_w2 = c1 * ci * k * k + c1
    o_fw = o_w2 + c2 * c1 * k * k + c2
    if part == "dead":
        ww[o_fw - c2:o_fw] = -1e3
    else:
        ww[{"conv1": 7, "conv2": o_w2 + 16 * c1 * k * k + 3, "fc": o_fw + cnn2_ref.dims(shape)[4] + 5}[part]] = np.nan
    engine.eval_set_cnn2(0, X, y, shape)
    out = engine.eval(ww, [0])
    assert triple(*out) == want(shape, ww, X, y)
    if part == "dead":
        assert int(out[1][0]) == int((y != int(np.argmax(ww[-C:].astype(np.float32)))).sum())
    else:
        assert int(out[2][0]) == len(y)  # a NaN logit flags its sample


def test_model_places_and_block_finish_eval(engine):
    """The model at BK_HOST_PINNED and BK_DEVICE gives BK_HOST's bits,
    bk_block_finish_eval on a CNN2 set the two-call sequence's, and a set of
    another kind in the same call is refused."""
    import torch
    shape = SMALL[3]
    c = case(shape)
    ev = ModelEvaluator(test=(c[1], c[2]), cnn2_shape=shape, engine=engine)
    assert ev.d == len(c[0]) and ev.test_error(c[0]) == cnn2_ref.counts(c[3], c[4], c[2])[0]
    base = engine.eval(c[0], [TEST])
    assert triple(*base) == want(shape, *c[:3]) and ev.near_ties[TEST] == base[2][0]
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
    assert triple(*two) == want(shape, g, c[1], c[2])
    engine.eval_set_softmax(0, c[1], c[2], shape[7])
    with pytest.raises(ValueError):  # a softmax set in the same call: mixed kinds
        engine.eval(c[0], [TEST, 0])
