"""GPU: the CNN2 verifier's rounds (bk_roni_cnn2_round_*), bit
for bit against tests/cnn2_ref.py (bk.h's arithmetic in numpy fp64) and against
bk_roni_cnn2_batches on the same model, rows and indices, at band heights that
put a band boundary inside the second pooled map.  No tolerances: scores are
compared as bytes, near-tie counts as integers."""
import ctypes
import functools

import numpy as np
import pytest

import cnn2_ref
from biscotti_amd import _lib as L
from biscotti_amd.roni import CNN2RONIValidator

pytestmark = pytest.mark.gpu

# the second pooled map: 4 x 2 (k = 3, pad 1); 3 x 1 (no padding: a halo row is never
# padding, the pool drops a row; F = 51: the fc tail); 3 x 2 (k = 2, pad 1; 3 conv2 row tiles)
S42, S31, S32 = (1, 16, 9, 3, 1, 2, 3, 2), (2, 20, 10, 3, 0, 3, 17, 3), (3, 12, 6, 2, 1, 18, 36, 2)


@functools.lru_cache(maxsize=None)
def case(shape, nv, nb, count, eps=0.0):
    """Model, set, rows, indices and the reference's scores and near-tie counts.
    eps: fc rows within eps of row 0 and no fc bias (near ties in the held verdicts)."""
    ww, X, y = cnn2_ref.make_case(shape, nv, sum(shape) + nv)
    if eps:
        (F, d), C = cnn2_ref.dims(shape)[4:], shape[7]
        fw = ww[d - C * F - C:d - C].reshape(C, F)
        fw[1:] = fw[0] + eps * fw[1:]
        ww[d - C:] = 0.0
    rng = np.random.default_rng(nb + 100 * count)
    deltas = 0.05 * rng.standard_normal((count, len(ww)))
    idx = rng.integers(0, nv, (count, 2, nb))
    idx[0, :, -1] = idx[0, :, 0]                   # repeats inside a batch
    idx[-1, 0, 0], idx[-1, 1, 0] = nv - 1, nv - 1  # the set's last sample: the begin's partial tile
    want, want_nt = cnn2_ref.roni(shape, ww, deltas, X, y, idx)
    for a in (ww, X, y, deltas, idx, want, want_nt):
        a.setflags(write=False)
    return ww, X, y, deltas, idx, want, want_nt


def score_at(engine, deltas, where, idx):
    """bk_roni_cnn2_round_score_batches on separately allocated rows at `where`."""
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
    st = L.lib().bk_roni_cnn2_round_score_batches(engine.ctx, (ctypes.c_void_p * n)(*ptrs), n, where,
                                                  idx.ctypes.data, idx.shape[2], out.ctypes.data,
                                                  nt.ctypes.data)
    return st, out, nt


@pytest.mark.parametrize("shape,band,nv,nb,count,where,eps", [
    (S42, 1, 33, 10, 2, L.BK_HOST, 0.0),
    (S42, 3, 33, 10, 2, L.BK_HOST, 0.0),           # bands of 3 + 1 rows
    (S42, 4, 33, 10, 2, L.BK_HOST, 0.0),           # one band
    (S31, 1, 33, 17, 3, L.BK_DEVICE, 0.0),         # two tiles per evaluation
    (S31, 2, 33, 17, 3, L.BK_DEVICE, 0.0),         # bands of 2 + 1 rows
    (S32, 1, 33, 10, 9, L.BK_HOST_PINNED, 0.0),    # more than one group
    (S32, 0, 33, 10, 9, L.BK_HOST_PINNED, 0.0),    # the library's choice
    (cnn2_ref.LFW, 1, 17, 10, 1, L.BK_HOST, 0.0),  # the verifier's own call
    (S31, 1, 33, 17, 3, L.BK_HOST, 2.0 ** -10),    # bit 1 of the held bytes: 10 of 33 near ties
])
def test_round_against_reference_and_batches(engine, shape, band, nv, nb, count, where, eps):
    ww, X, y, deltas, idx, want, want_nt = case(shape, nv, nb, count, eps)
    if eps:  # the held model's near ties: some samples, not all
        assert 0 < int(cnn2_ref.predict(shape, ww, X)[1].sum()) < nv
    v = CNN2RONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3, round_batches=True)
    batched = v.scores(ww, deltas, idx)
    batched_nt = v.last_near_ties
    v.set_band(band)
    try:
        v.begin_round(ww)
        if where == L.BK_HOST:
            got, nt = v.score_round(list(deltas), idx), v.last_near_ties
        else:
            st, got, nt = score_at(engine, deltas, where, idx)
            assert st == L.BK_OK, L.last_error()
    finally:
        v.set_band(0)
    print(shape, band, got, nt.ravel(), want, want_nt.ravel())
    assert got.tobytes() == want.tobytes() and np.array_equal(nt, want_nt)
    assert got.tobytes() == batched.tobytes() and np.array_equal(nt, batched_nt)


def test_round_state(engine):
    """A second begin replaces the model; set_validation ends the round; a
    refused score leaves it usable; bk_roni_cnn2_batches and bk_eval on a CNN2
    set return the same bytes before and after the round's calls; a
    default-built validator has no rounds."""
    shape, nv, nb = S31, 33, 10
    ww, X, y, deltas, idx = case(shape, nv, nb, 2)[:5]
    w2 = ww + 0.3 * np.random.default_rng(11).standard_normal(len(ww)) / 50
    v = CNN2RONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3, round_batches=True)
    engine.eval_set_cnn2(0, X, y, shape)
    before = (v.scores(ww, deltas, idx).tobytes(), [a.tobytes() for a in engine.eval(ww, [0])])
    for model in (ww, w2):
        v.begin_round(model)
        assert v.score_round(list(deltas), idx).tobytes() == \
            cnn2_ref.roni(shape, model, deltas, X, y, idx)[0].tobytes()
    bad = idx.copy()
    bad[1, 1, 4] = nv
    st, _, _ = score_at(engine, deltas, L.BK_HOST, bad)
    assert st == L.BK_EINVAL and "update 1, evaluation 1 (after), position 4" in L.last_error()
    assert v.score_round(list(deltas), idx).tobytes() == \
        cnn2_ref.roni(shape, w2, deltas, X, y, idx)[0].tobytes()
    assert before == (v.scores(ww, deltas, idx).tobytes(),
                      [a.tobytes() for a in engine.eval(ww, [0])])
    assert v.verify_update(type("U", (), {"NoisedDelta": deltas[0]})(), w2, round=True) in (True, False)
    assert v.rounds_begun == 2 and v.last_idx.shape == (1, 2, nv % nb)  # a drawn last batch
    plain = CNN2RONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=3)  # set_validation again
    st, _, _ = score_at(engine, deltas, L.BK_HOST, idx)
    assert st == L.BK_EINVAL and "no round" in L.last_error()
    with pytest.raises(ValueError):
        plain.begin_round(ww)


def test_round_nan_weight_and_dead_second_layer(engine):
    """A NaN conv2 weight in the held model (channel 16's features are NaN, so
    every logit is: every sample flagged, in the held verdicts and in `after`),
    and a delta that puts every conv2 bias at -1e3 (the logits are the fc biases)."""
    shape, nv, nb = S31, 33, 10
    ci, _, _, k, _, c1, c2, C = shape
    ww, X, y, _, idx = case(shape, nv, nb, 1)[:5]
    o_w2 = c1 * ci * k * k + c1
    o_fw = o_w2 + c2 * c1 * k * k + c2
    v = CNN2RONIValidator(X, y, shape, engine=engine, batch_size=nb, seed=1, round_batches=True)
    nan, dead = ww.copy(), ww.copy()
    nan[o_w2 + 16 * c1 * k * k + 3] = np.nan
    dead[o_fw - c2:o_fw] = -1e3
    v.set_band(1)
    try:
        for model, delta in ((nan, np.zeros(len(ww))), (ww, dead - ww)):
            v.begin_round(model)
            got = v.score_round([delta], idx)
            want, want_nt = cnn2_ref.roni(shape, model, delta[None], X, y, idx)
            assert got.tobytes() == want.tobytes() and np.array_equal(v.last_near_ties, want_nt)
            if model is nan:
                assert v.last_near_ties.tolist() == [[nb, nb]]
    finally:
        v.set_band(0)
