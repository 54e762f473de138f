"""MI355X: bk_grad_cnn2 against tests/grad_cnn2_ref.py at 1e-9 of
the norm-wise scale, loss and norm at the same relative gate; then the single
cases, the bitwise properties and the neighbouring kinds."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import cnn2_ref  # noqa: E402
import grad_cnn2_ref as R  # noqa: E402
import grad_ref  # noqa: E402
from biscotti_amd import _lib  # noqa: E402
from test_gpu_grad import Buf, _bits, _qsum_row  # noqa: E402

GATE, PREC, NN = 1e-9, 4, 24  # the project's fp64 gate, in units of the norm-wise scale
H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
# odd maps; c2 = 17, a k tail; k = 1, pad = 0, 16 classes; an even kernel, two row tiles of c1
SMALL = [(1, 5, 7, 3, 1, 1, 1, 2), (3, 6, 6, 3, 1, 5, 17, 3), (2, 4, 4, 1, 0, 3, 2, 16), (3, 8, 6, 2, 1, 18, 36, 2)]
CASES = [(s, n) for s in SMALL for n in (1, 2, 17)] + [(cnn2_ref.LFW, 1), (cnn2_ref.LFW, 10)]


@functools.lru_cache(maxsize=None)
def _case(shape, count):
    """(ww, X, y, idx, the restatement's (delta, loss, norm), scale); read-only."""
    ww, X, y = cnn2_ref.make_case(shape, NN, 3300 + count)
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
    engine.grad_set_cnn2(X, y, shape)
    l0 = engine.grad_stats()
    got = engine.grad_cnn2(ww, idx, precision=PREC)
    l1 = engine.grad_stats()
    _close(got, ref, scale)
    assert got[1].tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert [l1[0] - l0[0], l1[1] - l0[1]] == [4, 1]


@pytest.mark.parametrize("shape", [SMALL[3], SMALL[2]])  # d even: 16-byte stores; d odd: q's are not
def test_clipped_at_a_small_max_norm(engine, shape):
    ww, X, y, idx, ref, scale = _case(shape, 17)
    assert ref[2] > 0.05 and len(ww) % 2 == (shape == SMALL[2])
    engine.grad_set_cnn2(X, y, shape)
    got = engine.grad_cnn2(ww, idx, max_norm=0.05, precision=PREC)
    _close(got, R.step(shape, X, y, ww, idx, max_norm=0.05), scale)
    assert got[3] == engine.grad_cnn2(ww, idx)[3]  # norm_out: before clipping
    assert got[1].tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert abs(np.sqrt(np.sum(got[0] ** 2)) - 0.05) < 1e-6


def test_repeated_unsorted_idx_row_stride_and_null_idx(engine):
    shape = SMALL[1]
    ww, X, y = _case(shape, 17)[:3]
    buf = np.full((NN, X.shape[1] + 5), np.nan, dtype=np.float32)
    buf[:, :X.shape[1]] = X
    idx = np.random.default_rng(7).integers(0, NN, 17)
    assert len(np.unique(idx)) < 17 and (np.diff(idx) < 0).any()
    engine.grad_set_cnn2(buf[:, :X.shape[1]], y, shape)  # ldx = c_in h w + 5; the padding is never read
    _close(engine.grad_cnn2(ww, idx), R.step(shape, X, y, ww, idx), R.scale(shape, X, ww, idx))
    a = engine.grad_cnn2(ww, None, precision=PREC)
    b = engine.grad_cnn2(ww, np.arange(NN), precision=PREC)
    assert _bits(a[0]) == _bits(b[0]) and a[1].tolist() == b[1].tolist() and a[2:] == b[2:]
    _close(a, R.step(shape, X, y, ww), R.scale(shape, X, ww))


def test_noise_with_q_dead_second_layer_and_a_nan_weight_in_each_layer(engine):
    shape = SMALL[3]
    ci, h, w, k, pad, c1, c2, C = shape
    F, d = cnn2_ref.dims(shape)[4:]
    ww, X, y, idx = _case(shape, 17)[:4]
    noise = np.random.default_rng(9).uniform(-1e11, 1e11, len(ww))
    noise[5] = 1e300
    engine.grad_set_cnn2(X, y, shape)
    got = engine.grad_cnn2(ww, idx, noise=noise, precision=PREC)
    ref = R.step(shape, X, y, ww, idx, noise=noise)
    scale = R.scale(shape, X, ww, idx, np.delete(noise, 5))
    assert float(np.max(np.abs(np.delete(got[0] - ref[0], 5)))) <= GATE * scale
    assert got[1].tolist() == _qsum_row(engine, got[0]).tolist() == grad_ref.quantize(got[0], PREC).tolist()
    assert got[1][5] == -(1 << 63)
    o_b2 = c1 * ci * k * k + c1 + c2 * c1 * k * k
    dead = ww.copy()
    dead[o_b2:o_b2 + c2] = -100.0  # every second-layer pre-activation is negative
    got = engine.grad_cnn2(dead, idx)
    _close(got, R.step(shape, X, y, dead, idx), R.scale(shape, X, dead, idx))
    assert not got[0][:d - C].any() and got[0][-C:].all()
    for at in (3, o_b2 - 7, d - C - 2):  # conv1, conv2, fc
        bad = ww.copy()
        bad[at] = np.nan
        delta, q, _, _ = engine.grad_cnn2(bad, idx, precision=PREC)
        assert np.isnan(delta).all() and q.tolist() == [-(1 << 63)] * d


@pytest.mark.parametrize("shape,count", [(SMALL[1], 17), (cnn2_ref.LFW, 10)])
def test_where_forms_and_reruns_agree_bitwise(engine, shape, count):
    ww, X, y, idx = _case(shape, count)[:4]
    noise = np.random.default_rng(11).standard_normal(len(ww)) * 1e-3
    engine.grad_set_cnn2(X, y, shape)
    runs = []
    for where in (H, H, PIN, DEV):  # the host bits are the device bits
        w, nz = Buf(ww, where), Buf(noise, where)
        out, q = Buf(np.full(len(ww), 7.0), where), Buf(np.full(len(ww), 7, dtype=np.int64), where)
        loss, norm = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        engine.grad_cnn2_ptr(w.ptr, where, idx, 100.0, nz.ptr, PREC, out.ptr, q.ptr, loss, norm)
        runs.append((out.host(), q.host(), loss.value, norm.value))
    for r in runs[1:]:
        assert _bits(r[0]) == _bits(runs[0][0]) and r[1].tolist() == runs[0][1].tolist()
        assert r[2:] == runs[0][2:]


def test_kinds_the_batch_cap_and_the_stepper(engine):
    from biscotti_amd.train import CNN2Stepper
    shape = SMALL[1]
    ww, X, y, idx, ref, scale = _case(shape, 17)
    st = CNN2Stepper(X, y, shape, engine=engine)
    delta, q = st.private_fun(ww, idx, precision=PREC)
    _close((delta, q, st.loss, st.norm), ref, scale)
    wp, op = ww.ctypes.data, np.zeros(len(ww)).ctypes.data
    for call in (lambda: engine.grad_softmax_ptr(wp, H, idx, 100.0, None, -1, op, None),
                 lambda: engine.grad_logistic_ptr(wp, H, idx, 10, 1e-2, 0.01, None, -1, op, None),
                 lambda: engine.grad_cnn_ptr(wp, H, idx, 100.0, None, -1, op, None)):
        with pytest.raises(ValueError, match="two-layer CNN"):
            call()
    with pytest.raises(_lib.BKError, match="exceeds 1024"):
        engine.grad_cnn2_ptr(wp, H, np.zeros(_lib.BK_GRAD_CNN2_MAX_BATCH + 1, dtype=np.int64), 100.0, None, -1, op, None)
    engine.grad_set_cnn(np.zeros((4, 25), dtype=np.float32), np.zeros(4, dtype=np.int32), (5, 5, 3, 2, 1, 2))
    with pytest.raises(ValueError, match="CNN one"):
        engine.grad_cnn2_ptr(wp, H, idx, 100.0, None, -1, op, None)
    engine.grad_clear()
    with pytest.raises(ValueError, match="no resident training set"):
        engine.grad_cnn2_ptr(wp, H, idx, 100.0, None, -1, op, None)
