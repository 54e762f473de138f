"""GPU: the CNN verifier's rounds (bk_roni_cnn_round_*), bit
for bit against tests/cnn_ref.py (bk.h's arithmetic in numpy fp64) and against
bk_roni_cnn_batches on the same model, rows and indices.  No tolerances: scores
are compared as bytes, near-tie counts as integers."""
import ctypes

import numpy as np
import pytest

import cnn_ref
from biscotti_amd import _lib as L
from biscotti_amd.roni import CNNRONIValidator

pytestmark = pytest.mark.gpu

S49, S16, SHO = (5, 5, 3, 2, 1, 2), (7, 6, 3, 0, 3, 16), (9, 9, 5, 4, 16, 3)
TILES = 128  # tiles of one launch (CNN_ROUND_TILES)


def score_at(engine, deltas, where, idx):
    """bk_roni_cnn_round_score_batches on separately allocated rows at `where`."""
    import torch
    if where == L.BK_HOST:
        keep = [np.array(r) for r in deltas]
        ptrs = [r.ctypes.data for r in keep]
    else:
        keep = [torch.from_numpy(np.array(r)) for r in deltas]
        keep = [t.pin_memory() if where == L.BK_HOST_PINNED else t.cuda() for t in keep]
        torch.cuda.synchronize()
        ptrs = [t.data_ptr() for t in keep]
    n = len(ptrs)
    out, nt = np.empty(n), np.empty((n, 2), np.int32)
    st = L.lib().bk_roni_cnn_round_score_batches(engine.ctx, (ctypes.c_void_p * n)(*ptrs), n, where,
                                                 idx.ctypes.data, idx.shape[2], out.ctypes.data,
                                                 nt.ctypes.data)
    return st, out, nt


@pytest.mark.parametrize("shape,nv,nb,count,where", [
    (S49, 65, 1, 1, L.BK_HOST),                  # F = 49: the 4-feature tail and the chunk tail
    (S49, 16 * TILES + 1, 17, 3, L.BK_HOST),     # the begin takes two launches; two tiles per batch
    (S16, 65, 10, 9, L.BK_HOST_PINNED),          # 16 classes, no padding, two groups
    (SHO, 65, 17, 3, L.BK_DEVICE),               # 11 conv items per tile: the hand-off
    (SHO, 65, 10, 1, L.BK_HOST),
    (cnn_ref.MNIST, 17, 10, 1, L.BK_HOST),
])
def test_round_against_reference_and_batches(engine, shape, nv, nb, count, where):
    ww, X, y = cnn_ref.make_case(shape, nv, sum(shape) + nv)
    rng = np.random.default_rng(nb + 100 * count)
    deltas = 0.05 * rng.standard_normal((count, len(ww)))
    idx = rng.integers(0, nv, (count, 2, nb))
    idx[0, :, -1] = idx[0, :, 0]                 # repeats inside a batch
    idx[-1, 0, 0], idx[-1, 1, 0] = nv - 1, nv - 1  # the begin's partial last tile
    v = CNNRONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3)
    batched = v.scores(ww, deltas, idx)
    batched_nt = v.last_near_ties
    v.begin_round(ww)
    if where == L.BK_HOST:
        got, nt = v.score_round(list(deltas), idx), v.last_near_ties
    else:
        st, got, nt = score_at(engine, deltas, where, idx)
        assert st == L.BK_OK, L.last_error()
    want, want_nt = cnn_ref.roni(shape, ww, deltas, X, y, idx)
    print(shape, nv, nb, count, got, nt.ravel())
    assert got.tobytes() == want.tobytes() and np.array_equal(nt, want_nt)
    assert got.tobytes() == batched.tobytes() and np.array_equal(nt, batched_nt)


def test_round_state(engine):
    """A second begin replaces the model; set_validation ends the round; a
    refused score leaves it usable; bk_roni_cnn_batches and bk_eval on a CNN set
    return the same bytes before and after the round's calls."""
    shape, nv, nb = SHO, 65, 10
    ww, X, y = cnn_ref.make_case(shape, nv, 7)
    rng = np.random.default_rng(11)
    w2 = ww + 0.3 * rng.standard_normal(len(ww)) / 50
    deltas = 0.05 * rng.standard_normal((2, len(ww)))
    idx = rng.integers(0, nv, (2, 2, nb))
    v = CNNRONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3)
    engine.eval_set_cnn(0, X, y, shape)
    before = (v.scores(ww, deltas, idx).tobytes(), [a.tobytes() for a in engine.eval(ww, [0])])
    for model in (ww, w2):
        v.begin_round(model)
        assert v.score_round(list(deltas), idx).tobytes() == \
            cnn_ref.roni(shape, model, deltas, X, y, idx)[0].tobytes()
    bad = idx.copy()
    bad[1, 1, 4] = nv
    st, _, _ = score_at(engine, deltas, L.BK_HOST, bad)
    assert st == L.BK_EINVAL and "update 1, evaluation 1 (after), position 4" in L.last_error()
    assert v.score_round(list(deltas), idx).tobytes() == \
        cnn_ref.roni(shape, w2, deltas, X, y, idx)[0].tobytes()
    assert before == (v.scores(ww, deltas, idx).tobytes(),
                      [a.tobytes() for a in engine.eval(ww, [0])])
    assert v.verify_update(type("U", (), {"NoisedDelta": deltas[0]})(), w2, round=True) in (True, False)
    assert v.rounds_begun == 2 and v.last_idx.shape == (1, 2, nv % nb)  # a drawn last batch
    CNNRONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3)  # set_validation again
    st, _, _ = score_at(engine, deltas, L.BK_HOST, idx)
    assert st == L.BK_EINVAL and "no round" in L.last_error()


def test_round_nan_weight_and_dead_activations(engine):
    """A NaN conv weight in the held model (every logit NaN: class 0 predicted,
    every sample flagged, in the held verdicts and in `after`), and a delta
    that leaves every pre-activation negative (the logits are the fc biases)."""
    shape, nv, nb = SHO, 65, 10
    h, w, k, pad, co, C = shape
    ww, X, y = cnn_ref.make_case(shape, nv, 9)
    X = -np.abs(X)
    idx = np.random.default_rng(5).integers(0, nv, (1, 2, nb))
    v = CNNRONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=1)
    dead = ww.copy()
    dead[:co * k * k] = np.abs(dead[:co * k * k])
    dead[co * k * k:co * k * k + co] = -0.5
    nan = ww.copy()
    nan[3] = np.nan
    for model, delta in ((nan, np.zeros(len(ww))), (ww, dead - ww)):
        v.begin_round(model)
        got = v.score_round([delta], idx)
        want, want_nt = cnn_ref.roni(shape, model, delta[None], X, y, idx)
        assert got.tobytes() == want.tobytes() and np.array_equal(v.last_near_ties, want_nt)
        if model is nan:
            assert v.last_near_ties.tolist() == [[nb, nb]]
