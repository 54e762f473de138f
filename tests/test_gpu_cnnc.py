"""GPU: the one-layer cifar CNN's forward pass (bk_eval on a CNNC set,
bk_roni_cnnc_batches) against tests/cnnc_ref.py, the arithmetic
of include/bk.h in numpy fp64: equal wrong, err, scores and near-tie counts."""
import functools
import os

import numpy as np
import pytest

import cnnc_ref
from biscotti_amd import _lib as L
from biscotti_amd.evaluate import TEST, ModelEvaluator
from biscotti_amd.roni import CNNCRONIValidator

pytestmark = pytest.mark.gpu

# pad = k with the 4-feature and the chunk tail; h < k; an odd plane width; pad 0
# with 16 classes (and c_in = 1: bk_cnn_shape's ground); the largest c_in and k
SMALL = [(2, 5, 5, 3, 3, 2, 2), (2, 1, 4, 3, 1, 3, 2), (3, 6, 5, 3, 3, 5, 3), (1, 7, 6, 3, 0, 3, 16),
         (4, 9, 9, 5, 4, 20, 3)]
EVAL_CASES = [(s, nv, k) for s in SMALL for nv in (1, 15, 16, 17, 33) for k in (1, 2)] + \
             [(cnnc_ref.CIFAR, nv, k) for nv in (1, 17) for k in (1, 2)]
# chosen on the CPU so that the reference flags some of the 33 samples and not all (18, 15, 19, 13, 18)
EPS = dict(zip(SMALL, (2.0 ** -12, 2.0 ** -15, 2.0 ** -9, 2.0 ** -12, 2.0 ** -5)))
RONI_SHAPE = SMALL[2]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnnc_cifar_logits.npz")


@functools.lru_cache(maxsize=None)
def case(shape):
    """The shape's model and samples with the reference's per-sample verdicts."""
    ww, X, y = cnnc_ref.make_case(shape, 17 if shape == cnnc_ref.CIFAR else 33, sum(shape))
    pred, flag = cnnc_ref.predict(shape, ww, X)
    for a in (ww, X, y, pred, flag):
        a.setflags(write=False)
    return ww, X, y, pred, flag


def triple(err, wrong, near, i=0):
    return err[i].tobytes(), int(wrong[i]), int(near[i])


def want(shape, ww, X, y):
    err, wrong, near = cnnc_ref.counts(*cnnc_ref.predict(shape, ww, X), y)
    return np.float64(err).tobytes(), wrong, near


@pytest.mark.parametrize("shape,nv,nsets", EVAL_CASES)
def test_eval_against_reference(engine, shape, nv, nsets):
    c = case(shape)
    rows = [slice(0, nv), slice(len(c[2]) - nv, len(c[2]))][:nsets]  # the tile edges: nv
    for slot, r in enumerate(rows):
        engine.eval_set_cnnc(slot, c[1][r], c[2][r], shape)
    out = engine.eval(c[0], list(range(nsets)))
    for slot, r in enumerate(rows):
        err, wrong, near = cnnc_ref.counts(c[3][r], c[4][r], c[2][r])
        assert triple(*out, slot) == (np.float64(err).tobytes(), wrong, near)


@pytest.mark.parametrize("shape", SMALL)
def test_near_ties_counted(engine, shape):
    """fc rows within eps of row 0, no fc bias: some samples are near ties, some not."""
    ww, X, y = (a.copy() for a in case(shape)[:3])
    F, d = cnnc_ref.dims(shape)[2:]
    C = shape[6]
    fw = ww[d - C * F - C:d - C].reshape(C, F)
    fw[1:] = fw[0] + EPS[shape] * fw[1:]
    ww[d - C:] = 0.0
    ref = want(shape, ww, X, y)
    assert 0 < ref[2] < len(y)
    engine.eval_set_cnnc(0, X, y, shape)
    assert triple(*engine.eval(ww, [0])) == ref


@pytest.mark.parametrize("nb", [1, 10, 17])
@pytest.mark.parametrize("n", [1, 3])
def test_roni_batches_against_reference(engine, nb, n):
    ww, X, y = case(RONI_SHAPE)[:3]
    rng = np.random.default_rng(100 * nb + n)
    deltas = 0.05 * rng.standard_normal((n, len(ww)))
    idx = rng.integers(0, len(y), (n, 2, nb))  # drawn with repeats
    idx[0, 1, -1] = idx[0, 1, 0]
    v = CNNCRONIValidator(X, y, RONI_SHAPE, engine=engine, batch_size=nb, seed=3)
    got = v.scores(ww, deltas, idx)
    scores, near = cnnc_ref.roni(RONI_SHAPE, ww, deltas, X, y, idx)
    assert got.tobytes() == scores.tobytes()
    assert np.array_equal(v.last_near_ties, near)
    with pytest.raises(ValueError):
        v.begin_round(ww)


@pytest.mark.parametrize("part", ["conv", "fc", "dead"])
def test_nan_weight_and_dead_activations(engine, part):
    """One NaN weight in a layer: the call is BK_OK, the counts the restatement's.
    Conv biases of -1e3: every activation is dead, the logits are the fc biases."""
    shape = SMALL[2]
    ww, X, y = (a.copy() for a in case(shape)[:3])
    ci, _, _, k, _, co, C = shape
    o_cb = co * ci * k * k
    if part == "dead":
        ww[o_cb:o_cb + co] = -1e3
    else:
        ww[{"conv": 2 * ci * k * k + 11, "fc": o_cb + co + cnnc_ref.dims(shape)[2] + 5}[part]] = np.nan
    engine.eval_set_cnnc(0, X, y, shape)
    out = engine.eval(ww, [0])
    assert triple(*out) == want(shape, ww, X, y)
    if part == "dead":
        assert int(out[1][0]) == int((y != int(np.argmax(ww[-C:].astype(np.float32)))).sum())
    else:
        assert int(out[2][0]) == len(y)  # a NaN logit flags its sample


def test_single_channel_equals_one_layer_entries(engine):
    """c_in = 1 at a shape bk_cnn_shape accepts: the same triples from both kernels."""
    shape = SMALL[3]
    ww, X, y = case(shape)[:3]
    engine.eval_set_cnnc(0, X, y, shape)
    engine.eval_set_cnn(1, X, y, shape[1:])
    assert triple(*engine.eval(ww, [0])) == triple(*engine.eval(ww, [1])) == want(shape, ww, X, y)


def test_model_places_and_block_finish_eval(engine):
    """The model at BK_HOST_PINNED and BK_DEVICE gives BK_HOST's bits,
    bk_block_finish_eval on a CNNC set the two-call sequence's, and a set of
    another kind in the same call is refused."""
    import torch
    shape = SMALL[2]
    c = case(shape)
    ev = ModelEvaluator(test=(c[1], c[2]), cnnc_shape=shape, engine=engine)
    assert ev.d == len(c[0]) and ev.test_error(c[0]) == cnnc_ref.counts(c[3], c[4], c[2])[0]
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
    engine.eval_set_softmax(0, c[1], c[2], shape[6])
    with pytest.raises(ValueError):  # a softmax set in the same call: mixed kinds
        engine.eval(c[0], [TEST, 0])


def test_against_torch(engine):
    """torch's fp32 logits of the reference's CIFARCNNModel (tests/golden/
    gen_cnnc_goldens.py): every sample the GPU does not flag has torch's
    prediction, and at most half are flagged."""
    gold = np.load(GOLDEN)
    ww, X, _ = cnnc_ref.make_case(cnnc_ref.CIFAR, len(gold["pred"]), int(gold["seed"]))
    # with torch's predictions as the labels, wrong counts the disagreements
    engine.eval_set_cnnc(0, X, gold["pred"], cnnc_ref.CIFAR)
    _, wrong, near = engine.eval(ww, [0])
    flag = np.array([engine.eval_set_cnnc(1, X[i:i + 1], gold["pred"][i:i + 1], cnnc_ref.CIFAR) or
                     engine.eval(ww, [1])[1:] for i in range(len(X))]).reshape(len(X), 2)
    print("flagged", near[0], "of", len(X), "disagreeing", wrong[0], "golden share", float(gold["share"]))
    assert int(flag[:, 1].sum()) == near[0] and int(flag[:, 0].sum()) == wrong[0]
    assert not np.any((flag[:, 0] == 1) & (flag[:, 1] == 0))
    assert near[0] <= 32
