"""MI355X: the one-layer CNN's gradient step (bk_grad_cnn) against the numpy
restatement (tests/grad_cnn_ref.py) at 1e-9 of the norm-wise scale, loss and
norm at the same relative gate, and against the torch goldens under their
recorded gates.  Then the single cases (idx, noise and q, the clip, dead
activations, a NaN), the bitwise properties and the neighbouring state."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_ref  # noqa: E402
import grad_cnn_ref as R  # noqa: E402
import grad_ref  # noqa: E402
from biscotti_amd import _lib  # noqa: E402
from test_gpu_grad import Buf, _bits, _qsum_row  # noqa: E402

GATE = 1e-9  # the project's fp64 gate, in units of the norm-wise scale
H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
PREC, NN = 4, 40
# one channel, F = 49, tails of every MFMA block; no padding, 16 classes, h != w;
# k = 5 with pad 4, 16 channels
SMALL = [(5, 5, 3, 2, 1, 2), (7, 6, 3, 0, 3, 16), (9, 9, 5, 4, 16, 3)]
# the largest shape tiles by 8 positions, not 16: one tile and a tail, across the boundary
LARGE = (64, 64, 5, 4, 16, 2)
CASES = [(s, n) for s in SMALL for n in (1, 15, 16, 17, 33)] + \
    [(cnn_ref.MNIST, 1), (cnn_ref.MNIST, 10), (cnn_ref.MNIST, 17), (LARGE, 9)]


@functools.lru_cache(maxsize=None)
def _case(shape, count):
    """(ww, X, y, idx, the restatement's (delta, loss, norm), scale); read-only."""
    ww, X, y = cnn_ref.make_case(shape, NN, 3100 + count)
    idx = np.random.default_rng(count).permutation(NN)[:count].astype(np.int64)
    return ww, X, y, idx, R.step(shape, X, y, ww, idx), R.scale(shape, X, ww, idx)


def _close(got, ref, scale):
    delta, _, loss, norm = got
    dev = float(np.max(np.abs(delta - ref[0])) / scale)
    print("deviation", dev, "loss", loss, ref[1], "norm", norm, ref[2])
    assert dev <= GATE
    assert abs(loss - ref[1]) <= GATE * max(abs(ref[1]), 1.0)
    assert abs(norm - ref[2]) <= GATE * max(ref[2], scale)


@pytest.mark.parametrize("shape,count", CASES)
def test_against_the_restatement(engine, shape, count):
    ww, X, y, idx, ref, scale = _case(shape, count)
    engine.grad_set_cnn(X, y, shape)
    l0 = engine.grad_stats()
    got = engine.grad_cnn(ww, idx, precision=PREC)
    l1 = engine.grad_stats()
    _close(got, ref, scale)
    assert got[1].tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert [l1[0] - l0[0], l1[1] - l0[1]] == [3, 1]


@pytest.mark.parametrize("name", R.golden_names())
def test_against_the_torch_goldens(engine, name):
    c = R.load_golden(name)
    p = c["p"]
    engine.grad_set_cnn(c["X"], c["y"], cnn_ref.MNIST)
    got = engine.grad_cnn(c["ww"], c["idx"], precision=PREC)
    delta, q, loss, norm = got
    # the clip included: the restatement at the fp64 gate, then torch at its own
    _close(got, R.step(cnn_ref.MNIST, c["X"], c["y"], c["ww"], c["idx"]), p["scale"])
    assert q.tolist() == grad_ref.quantize(delta, PREC).tolist()
    dev = float(np.max(np.abs(delta - c["delta"])) / p["scale"])
    print(name, "against torch", dev, "gate", p["gate"], "norm", norm, c["norm"])
    assert dev <= p["gate"]
    assert abs(norm - c["norm"]) <= p["gate"] * max(c["norm"], p["scale"])
    assert abs(loss - c["loss"]) <= p["gate"] * max(abs(c["loss"]), 1.0)
    # the clipped case: norm_out is the norm before clipping, the delta is scaled
    assert (norm > 100.0) == (name == "grad_cnn_clip")
    assert np.sqrt(np.sum(delta * delta)) <= 100.0 * (1 + 1e-12)


@pytest.mark.parametrize("shape", [SMALL[0], SMALL[2]])  # d even: 16-byte stores; d odd: q's are not
def test_clipped_at_a_small_max_norm(engine, shape):
    ww, X, y, idx, ref, scale = _case(shape, 17)
    assert ref[2] > 0.05
    engine.grad_set_cnn(X, y, shape)
    got = engine.grad_cnn(ww, idx, max_norm=0.05, precision=PREC)
    _close(got, R.step(shape, X, y, ww, idx, max_norm=0.05), scale)
    assert got[3] == engine.grad_cnn(ww, idx)[3]  # norm_out: before clipping
    assert got[1].tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert abs(np.sqrt(np.sum(got[0] ** 2)) - 0.05) < 1e-6


def test_repeated_unsorted_idx_and_row_stride(engine):
    shape = SMALL[2]
    ww, X, y = _case(shape, 33)[:3]
    buf = np.full((NN, X.shape[1] + 5), np.nan, dtype=np.float32)
    buf[:, :X.shape[1]] = X
    idx = np.random.default_rng(7).integers(0, NN, 33)
    assert len(np.unique(idx)) < 33 and (np.diff(idx) < 0).any()
    engine.grad_set_cnn(buf[:, :X.shape[1]], y, shape)  # ldx = h w + 5; the padding is never read
    _close(engine.grad_cnn(ww, idx), R.step(shape, X, y, ww, idx), R.scale(shape, X, ww, idx))


def test_null_idx_is_every_row(engine):
    shape = SMALL[1]
    ww, X, y = _case(shape, 17)[:3]
    engine.grad_set_cnn(X, y, shape)
    a = engine.grad_cnn(ww, None, precision=PREC)
    b = engine.grad_cnn(ww, np.arange(NN), precision=PREC)
    assert _bits(a[0]) == _bits(b[0]) and a[1].tolist() == b[1].tolist() and a[2:] == b[2:]
    _close(a, R.step(shape, X, y, ww), R.scale(shape, X, ww))


def test_noise_and_q_is_the_quantised_sum_of_the_one_row(engine):
    shape = SMALL[2]
    ww, X, y, idx = _case(shape, 17)[:4]
    noise = np.random.default_rng(9).uniform(-1e11, 1e11, len(ww))
    noise[5] = 1e300
    engine.grad_set_cnn(X, y, shape)
    got = engine.grad_cnn(ww, idx, noise=noise, precision=PREC)
    ref = R.step(shape, X, y, ww, idx, noise=noise)
    scale = R.scale(shape, X, ww, idx, np.delete(noise, 5))
    assert float(np.max(np.abs(np.delete(got[0] - ref[0], 5)))) <= GATE * scale
    assert got[1].tolist() == _qsum_row(engine, got[0]).tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert got[1][5] == -(1 << 63)


def test_dead_activations_and_a_nan_weight(engine):
    shape = SMALL[2]
    h, w, k, pad, co, C = shape
    ww, X, y, idx = _case(shape, 17)[:4]
    dead = ww.copy()
    dead[co * k * k:co * k * k + co] = -100.0  # every pre-activation is negative
    engine.grad_set_cnn(X, y, shape)
    got = engine.grad_cnn(dead, idx)
    _close(got, R.step(shape, X, y, dead, idx), R.scale(shape, X, dead, idx))
    assert not got[0][:co * k * k + co].any() and got[0][-C:].all()
    bad = ww.copy()
    bad[3] = np.nan
    delta, q, _, _ = engine.grad_cnn(bad, idx, precision=PREC)
    assert np.isnan(delta).all() and q.tolist() == [-(1 << 63)] * len(ww)


@pytest.mark.parametrize("shape,count", [(SMALL[0], 17), (cnn_ref.MNIST, 10)])
def test_where_forms_and_reruns_agree_bitwise(engine, shape, count):
    ww, X, y, idx = _case(shape, count)[:4]
    noise = np.random.default_rng(11).standard_normal(len(ww)) * 1e-3
    engine.grad_set_cnn(X, y, shape)
    runs = []
    for where in (H, H, PIN, DEV):  # the host bits are the device bits
        w, nz = Buf(ww, where), Buf(noise, where)
        out, q = Buf(np.full(len(ww), 7.0), where), Buf(np.full(len(ww), 7, dtype=np.int64), where)
        loss, norm = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        engine.grad_cnn_ptr(w.ptr, where, idx, 100.0, nz.ptr, PREC, out.ptr, q.ptr, loss, norm)
        runs.append((out.host(), q.host(), loss.value, norm.value))
    for r in runs[1:]:
        assert _bits(r[0]) == _bits(runs[0][0]) and r[1].tolist() == runs[0][1].tolist()
        assert r[2:] == runs[0][2:]


def test_neighbours_kinds_limits_and_stepper(engine):
    from biscotti_amd.roni import CNNRONIValidator, RONIValidator
    from biscotti_amd.train import CNNStepper
    shape = SMALL[2]
    ww, X, y, idx, ref, scale = _case(shape, 17)
    engine.eval_set_cnn(2, X, y, shape)
    v = CNNRONIValidator(X, y, shape, engine=engine, seed=1)
    deltas = np.random.default_rng(13).standard_normal((3, len(ww))) * 0.05
    bidx = v.draw_batches(3)
    Xl = np.random.default_rng(14).standard_normal((50, 6))
    lv = RONIValidator(Xl, np.sign(Xl[:, 0]), engine=engine)
    lv.begin_round(np.ones(6))
    dl = np.random.default_rng(15).standard_normal((4, 6))
    before = [a.copy() for a in engine.eval(ww, [2])], v.scores(ww, deltas, bidx), lv.score_round(dl).copy()
    st = CNNStepper(X, y, shape, engine=engine)
    delta, q = st.private_fun(ww, idx, precision=PREC)
    _close((delta, q, st.loss, st.norm), ref, scale)
    after = engine.eval(ww, [2]), v.scores(ww, deltas, bidx), lv.score_round(dl)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0]))
    assert _bits(before[1]) == _bits(after[1]) and _bits(before[2]) == _bits(after[2])
    engine.eval_clear(2)
    # one of the other kind; the batch limit; bk_grad_clear
    out = np.zeros(len(ww))
    for call in (lambda: engine.grad_softmax_ptr(ww.ctypes.data, H, idx, 100.0, None, -1, out.ctypes.data, None),
                 lambda: engine.grad_logistic_ptr(ww.ctypes.data, H, idx, 10, 1e-2, 0.01, None, -1,
                                                  out.ctypes.data, None)):
        with pytest.raises(ValueError, match="CNN"):
            call()
    with pytest.raises(_lib.BKError) as ei:
        engine.grad_cnn_ptr(ww.ctypes.data, H, np.zeros(4097, dtype=np.int64), 100.0, None, -1,
                            out.ctypes.data, None)
    assert ei.value.status == _lib.BK_ENOTSUP
    s = np.zeros((4, 3), dtype=np.float32)
    engine.grad_set_softmax(s, np.zeros(4, dtype=np.int64), 2)
    with pytest.raises(ValueError, match="softmax"):
        engine.grad_cnn_ptr(ww.ctypes.data, H, idx, 100.0, None, -1, out.ctypes.data, None)
    engine.grad_clear()
    with pytest.raises(ValueError, match="no resident training set"):
        engine.grad_cnn_ptr(ww.ctypes.data, H, idx, 100.0, None, -1, out.ctypes.data, None)
