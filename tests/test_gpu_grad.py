"""MI355X: the gradient step (bk_grad_*) against the numpy restatement
(tests/grad_ref.py) at 1e-9 of the norm-wise scale and against the reference-run
goldens (tests/golden/gen_grad_goldens.py): the logistic ones at 1e-9 x scale,
the torch fp32 softmax ones at (d_in + count + 8) 2^-24 x scale.  Then the
bitwise properties: the three `where` forms, idx = NULL against arange, two
runs, the mapped against the copied host outputs (d = 784 / 785), q against
bk_quantized_sum_device; the neighbouring state; the launch counts.

There is one softmax route (two launches), so no route-against-route check.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import grad_cases as GC  # noqa: E402
import grad_ref as R  # noqa: E402
from biscotti_amd import _lib  # noqa: E402

H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
PREC = 4
INT64_MIN = -(1 << 63)


class Buf:
    """A numpy array's content at `where`, with its pointer; host() reads it back."""

    def __init__(self, a, where):
        a = np.ascontiguousarray(a)
        self.where = where
        if where == H:
            self.t = a.copy()
            self.ptr = self.t.ctypes.data
        elif where == PIN:
            self.t = torch.from_numpy(a.copy()).pin_memory()
            self.ptr = self.t.data_ptr()
        else:
            self.t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            self.ptr = self.t.data_ptr()

    def host(self):
        return self.t.copy() if self.where == H else self.t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64).tolist()


def _at(engine, kind, where, ww, idx, noise, precision, **kw):
    """A gradient call with the model, noise and outputs at `where`:
    (delta, q or None, loss, norm or None)."""
    d = len(ww)
    w = Buf(ww, where)
    nz = Buf(noise, where) if noise is not None else None
    out = Buf(np.full(d, 7.0), where)
    q = Buf(np.full(d, 7, dtype=np.int64), where) if precision >= 0 else None
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
    loss, norm = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    if kind == "logistic":
        engine.grad_logistic_ptr(w.ptr, where, ix, kw["batch"], kw.get("alpha", 1e-2),
                                 kw.get("lammy", 0.01), nz.ptr if nz else None, precision, out.ptr,
                                 q.ptr if q else None, loss)
        norm = None
    else:
        engine.grad_softmax_ptr(w.ptr, where, ix, kw.get("max_norm", 100.0),
                                nz.ptr if nz else None, precision, out.ptr, q.ptr if q else None,
                                loss, norm)
    return out.host(), q.host() if q else None, loss.value, norm.value if norm else None


@functools.lru_cache(maxsize=None)
def _logistic_ref(name):
    c = GC.load(name)
    p = c["p"]
    delta, loss = R.logistic(c["X"], c["y"], c["ww"], c["idx"], p["batch"], p["alpha"], p["lammy"],
                             c["noise"])
    scale = R.logistic_scale(c["X"], c["ww"], c["idx"], p["batch"], p["alpha"], p["lammy"],
                             c["noise"])
    return delta, loss, scale


@functools.lru_cache(maxsize=None)
def _softmax_ref(name):
    c = GC.load(name)
    delta, loss, norm = R.softmax(c["X"], c["y"], c["ww"], c["idx"], c["p"]["C"])
    return delta, loss, norm, R.softmax_scale(c["X"], c["idx"])


# ---- the goldens and the restatement -------------------------------------------
@pytest.mark.parametrize("name", GC.names("logistic"))
def test_logistic_cases(engine, name):
    c = GC.load(name)
    p = c["p"]
    ref, ref_loss, scale = _logistic_ref(name)
    engine.grad_set_logistic(c["X"], c["y"])
    l0 = engine.grad_stats()
    delta, q, loss = engine.grad_logistic(c["ww"], c["idx"], p["batch"], p["alpha"], p["lammy"],
                                          c["noise"], PREC)
    l1 = engine.grad_stats()
    dev_ref = float(np.max(np.abs(delta - ref)) / scale)
    dev_gold = float(np.max(np.abs(delta - c["delta"])) / scale)
    print(name, "against grad_ref", dev_ref, "against the reference", dev_gold, "loss", loss,
          c["loss"])
    assert np.isfinite(delta).all()
    assert dev_ref <= GC.FP64_GATE
    assert dev_gold <= GC.FP64_GATE
    assert abs(loss - ref_loss) <= GC.FP64_GATE * max(abs(ref_loss), 1.0)
    assert abs(loss - c["loss"]) <= GC.FP64_GATE * max(abs(c["loss"]), 1.0)
    assert q.tolist() == R.quantize(delta, PREC).tolist()
    assert [l1[0] - l0[0], l1[1] - l0[1]] == [1, 1]  # one launch per logistic call


def test_logistic_repeated_unsorted_idx_and_row_stride(engine):
    c = GC.load("grad_lg_700x100")
    nn, d = c["X"].shape
    buf = np.full((nn, d + 4), np.nan)
    buf[:, :d] = c["X"]
    Xv = buf[:, :d]  # ldx = d + 4; the padding is never read
    idx = np.random.default_rng(31).integers(0, nn, 700)
    assert len(np.unique(idx)) < 700 and (np.diff(idx) < 0).any()
    noise = np.random.default_rng(32).standard_normal(d) * 1e-3
    engine.grad_set_logistic(Xv, c["y"])
    delta, _, loss = engine.grad_logistic(c["ww"], idx, 700, noise=noise)
    ref, ref_loss = R.logistic(c["X"], c["y"], c["ww"], idx, 700, noise=noise)
    scale = R.logistic_scale(c["X"], c["ww"], idx, 700, noise=noise)
    dev = float(np.max(np.abs(delta - ref)) / scale)
    print("700 x 100 repeated", dev)
    assert dev <= GC.FP64_GATE
    assert abs(loss - ref_loss) <= GC.FP64_GATE * max(abs(ref_loss), 1.0)


def test_logistic_margins_are_finite_on_both_sides(engine):
    c = GC.load("grad_lg_margins")
    t = c["y"][c["idx"]] * (c["X"][c["idx"]] @ c["ww"])
    assert (t > 700).any() and (t < -700).any()
    engine.grad_set_logistic(c["X"], c["y"])
    delta, _, loss = engine.grad_logistic(c["ww"], c["idx"], c["p"]["batch"])
    assert np.isfinite(delta).all() and np.isfinite(loss)


@pytest.mark.parametrize("name", GC.names("softmax"))
def test_softmax_cases(engine, name):
    c = GC.load(name)
    p = c["p"]
    ref, ref_loss, ref_norm, scale = _softmax_ref(name)
    gate = GC.softmax_gate(p["din"], p["count"])
    engine.grad_set_softmax(c["X"], c["y"], p["C"])
    l0 = engine.grad_stats()
    delta, q, loss, norm = engine.grad_softmax(c["ww"], c["idx"], precision=PREC)
    l1 = engine.grad_stats()
    dev_ref = float(np.max(np.abs(delta - ref)) / scale)
    dev_gold = float(np.max(np.abs(delta - c["delta"])) / scale)
    print(name, "against grad_ref", dev_ref, "against the reference", dev_gold, "gate", gate,
          "norm", norm, c["norm"], "loss", loss, c["loss"])
    assert dev_ref <= GC.FP64_GATE
    assert dev_gold <= gate
    assert abs(norm - ref_norm) <= GC.FP64_GATE * max(ref_norm, scale)
    assert abs(norm - c["norm"]) <= gate * max(c["norm"], scale)
    assert abs(loss - ref_loss) <= GC.FP64_GATE * max(abs(ref_loss), 1.0)
    assert abs(loss - c["loss"]) <= gate * max(abs(c["loss"]), 1.0)
    if "xscale" in p:
        assert norm > 100.0  # the clip acted
    assert q.tolist() == R.quantize(delta, PREC).tolist()
    assert 1 <= l1[0] - l0[0] <= 2 and l1[1] - l0[1] == 1  # at most two launches


def test_softmax_noise_and_repeats(engine):
    c = GC.load("grad_sm_257x70x3")
    p = c["p"]
    idx = np.random.default_rng(41).integers(0, p["nn"], 300)
    noise = np.random.default_rng(42).standard_normal(len(c["ww"])) * 1e-2
    engine.grad_set_softmax(c["X"], c["y"], p["C"])
    delta, _, loss, norm = engine.grad_softmax(c["ww"], idx, noise=noise)
    ref, ref_loss, ref_norm = R.softmax(c["X"], c["y"], c["ww"], idx, p["C"], noise=noise)
    scale = R.softmax_scale(c["X"], idx, noise)
    assert float(np.max(np.abs(delta - ref)) / scale) <= GC.FP64_GATE
    assert abs(norm - ref_norm) <= GC.FP64_GATE * max(ref_norm, scale)
    assert abs(loss - ref_loss) <= GC.FP64_GATE * max(abs(ref_loss), 1.0)


# ---- bitwise -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grad_lg_credit", "grad_lg_257x33", "grad_lg_700x100"])
def test_logistic_where_forms_and_reruns_agree_bitwise(engine, name):
    c = GC.load(name)
    noise = np.random.default_rng(51).standard_normal(len(c["ww"])) * 1e-3
    engine.grad_set_logistic(c["X"], c["y"])
    runs = [_at(engine, "logistic", w, c["ww"], c["idx"], noise, PREC, batch=c["p"]["batch"])
            for w in (H, H, PIN, DEV)]
    for r in runs[1:]:
        assert _bits(r[0]) == _bits(runs[0][0])
        assert r[1].tolist() == runs[0][1].tolist()
        assert r[2] == runs[0][2]


@pytest.mark.parametrize("name", ["grad_sm_7x24x2", "grad_sm_mnist", "grad_sm_257x70x3"])
def test_softmax_where_forms_and_reruns_agree_bitwise(engine, name):
    c = GC.load(name)
    noise = np.random.default_rng(52).standard_normal(len(c["ww"])) * 1e-3
    engine.grad_set_softmax(c["X"], c["y"], c["p"]["C"])
    runs = [_at(engine, "softmax", w, c["ww"], c["idx"], noise, PREC) for w in (H, H, PIN, DEV)]
    for r in runs[1:]:
        assert _bits(r[0]) == _bits(runs[0][0])
        assert r[1].tolist() == runs[0][1].tolist()
        assert (r[2], r[3]) == (runs[0][2], runs[0][3])


def test_null_idx_is_arange(engine):
    c = GC.load("grad_lg_full600")
    engine.grad_set_logistic(c["X"], c["y"])
    a = engine.grad_logistic(c["ww"], None, 600, precision=PREC)
    b = engine.grad_logistic(c["ww"], np.arange(600), 600, precision=PREC)
    assert _bits(a[0]) == _bits(b[0]) and a[1].tolist() == b[1].tolist() and a[2] == b[2]
    c = GC.load("grad_sm_7x24x2")
    engine.grad_set_softmax(c["X"], c["y"], c["p"]["C"])
    a = engine.grad_softmax(c["ww"], None, precision=PREC)
    b = engine.grad_softmax(c["ww"], np.arange(c["p"]["nn"]), precision=PREC)
    assert _bits(a[0]) == _bits(b[0]) and a[1].tolist() == b[1].tolist() and a[2:] == b[2:]


@pytest.mark.parametrize("d", [784, 785])
def test_mapped_and_copied_host_outputs_are_the_kernels_bits(engine, d):
    # host outputs of up to 784 entries are stored into mapped memory, larger
    # ones copied; a device output is written where it is.  All the same bits
    rng = np.random.default_rng(60 + d)
    X = rng.standard_normal((40, d))
    y = rng.choice([-1.0, 1.0], 40)
    ww = rng.standard_normal(d) * 0.05
    idx = rng.permutation(40)[:10]
    engine.grad_set_logistic(X, y)
    host = _at(engine, "logistic", H, ww, idx, None, PREC, batch=10)
    dev = _at(engine, "logistic", DEV, ww, idx, None, PREC, batch=10)
    assert _bits(host[0]) == _bits(dev[0]) and host[1].tolist() == dev[1].tolist()
    ref, _ = R.logistic(X, y, ww, idx, 10)
    assert np.max(np.abs(host[0] - ref)) <= GC.FP64_GATE * R.logistic_scale(X, ww, idx, 10)
    # the softmax form: d = C (d_in + 1) = 2 x 392 and 5 x 157
    C, din = (2, 391) if d == 784 else (5, 156)
    Xf = rng.standard_normal((20, din)).astype(np.float32)
    yi = rng.integers(0, C, 20)
    wm = rng.standard_normal(d) * 0.05
    engine.grad_set_softmax(Xf, yi, C)
    host = _at(engine, "softmax", H, wm, None, None, PREC)
    dev = _at(engine, "softmax", DEV, wm, None, None, PREC)
    assert _bits(host[0]) == _bits(dev[0]) and host[1].tolist() == dev[1].tolist()
    assert host[2:] == dev[2:]


def _qsum_row(engine, row):
    """bk_quantized_sum_device on the one row `row`."""
    d = len(row)
    dx = torch.from_numpy(np.ascontiguousarray(row)[None]).cuda()
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.empty(d, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    engine.quantized_sum_ptr(dx.data_ptr(), _lib.BK_F64, 1, d, d, idx.data_ptr(), 1, PREC,
                             s.data_ptr(), None)
    engine.synchronize()
    return s.cpu().numpy()


def test_q_is_the_quantised_sum_of_the_one_row(engine):
    c = GC.load("grad_lg_257x33")
    d = len(c["ww"])
    noise = np.random.default_rng(71).uniform(-1e11, 1e11, d)  # entries up to 1e11
    noise[5] = 1e300
    engine.grad_set_logistic(c["X"], c["y"])
    delta, q, _ = engine.grad_logistic(c["ww"], c["idx"], 257, noise=noise, precision=PREC)
    assert np.abs(delta).max() > 1e10
    assert q.tolist() == _qsum_row(engine, delta).tolist() == R.quantize(delta, PREC).tolist()
    assert q[5] == INT64_MIN
    # a NaN in the model: BK_OK, an all-NaN delta, every q the integer indefinite
    w = c["ww"].copy()
    w[3] = np.nan
    delta, q, _ = engine.grad_logistic(w, c["idx"], 257, precision=PREC)
    assert np.isnan(delta).all()
    assert q.tolist() == _qsum_row(engine, delta).tolist() == [INT64_MIN] * d
    c = GC.load("grad_sm_7x24x2")
    engine.grad_set_softmax(c["X"], c["y"], c["p"]["C"])
    w = c["ww"].copy()
    w[3] = np.nan
    delta, q, _, _ = engine.grad_softmax(w, c["idx"], precision=PREC)
    assert np.isnan(delta).all()
    assert q.tolist() == _qsum_row(engine, delta).tolist() == [INT64_MIN] * len(w)


def test_no_precision_no_q(engine):
    c = GC.load("grad_lg_credit")
    engine.grad_set_logistic(c["X"], c["y"])
    delta, q, _ = engine.grad_logistic(c["ww"], c["idx"], 10)
    ref, _, scale = _logistic_ref("grad_lg_credit")
    assert q is None and np.max(np.abs(delta - ref)) <= GC.FP64_GATE * scale


# ---- the checks that need a resident set ---------------------------------------
def test_checks_behind_the_resident_set(engine):
    c = GC.load("grad_lg_credit")
    d = len(c["ww"])
    w, out = np.zeros(d), np.zeros(d)
    idx = np.arange(10, dtype=np.int64)

    def lg(ix=idx):
        engine.grad_logistic_ptr(w.ctypes.data, H, ix, 10, 1e-2, 0.01, None, -1, out.ctypes.data, None)

    def sm(ix=idx):
        engine.grad_softmax_ptr(w.ctypes.data, H, ix, 100.0, None, -1, out.ctypes.data, None)

    engine.grad_clear()
    with pytest.raises(ValueError, match="no resident training set"):
        lg()
    engine.grad_set_logistic(c["X"], c["y"])
    with pytest.raises(ValueError, match="logistic"):
        sm()
    with pytest.raises(ValueError, match="count=0"):
        lg(np.zeros(0, dtype=np.int64))
    bad = idx.copy()
    bad[7] = len(c["X"])
    with pytest.raises(ValueError, match=r"idx\[7\]=500"):
        lg(bad)
    bad[7] = -1
    with pytest.raises(ValueError, match=r"idx\[7\]=-1"):
        lg(bad)
    with pytest.raises(_lib.BKError) as ei:
        lg(np.zeros(65537, dtype=np.int64))
    assert ei.value.status == _lib.BK_ENOTSUP
    lg()  # and the set still serves
    engine.grad_clear()
    with pytest.raises(ValueError, match="no resident training set"):
        lg()
    assert not out.any() or np.isfinite(out).all()


# ---- neighbouring state ------------------------------------------------------------
def test_eval_sets_and_a_live_roni_round_are_untouched(engine):
    from biscotti_amd.roni import RONIValidator
    c = GC.load("grad_lg_credit")
    X, y, ww = c["X"], c["y"].astype(np.float64), c["ww"]
    engine.eval_set_logistic(3, X[:200], y[:200])
    before_eval = [a.copy() for a in engine.eval(ww, [3])]
    v = RONIValidator(X[200:400], y[200:400], engine=engine)
    deltas = np.random.default_rng(81).standard_normal((5, len(ww))) * 0.1
    v.begin_round(ww)
    before_round = v.score_round(deltas).copy()
    engine.grad_set_logistic(X, y)
    engine.grad_logistic(ww, c["idx"], 10, precision=PREC)
    s = GC.load("grad_sm_7x24x2")
    engine.grad_set_softmax(s["X"], s["y"], s["p"]["C"])
    engine.grad_softmax(s["ww"], s["idx"], precision=PREC)
    after_round = v.score_round(deltas)  # the round begun before is still live
    after_eval = engine.eval(ww, [3])
    assert _bits(after_round) == _bits(before_round)
    for a, b in zip(before_eval, after_eval):
        assert a.tobytes() == b.tobytes()
    engine.eval_clear(3)


def test_steppers(engine):
    from biscotti_amd.train import LogisticStepper, SoftmaxStepper
    c = GC.load("grad_lg_noise")
    p = c["p"]
    st = LogisticStepper(c["X"], c["y"], p["batch"], engine=engine)
    delta, q = st.private_fun(c["ww"], c["idx"], c["noise"], precision=PREC)
    ref, _, scale = _logistic_ref("grad_lg_noise")
    assert np.max(np.abs(delta - c["delta"])) <= GC.FP64_GATE * scale
    assert q.tolist() == R.quantize(delta, PREC).tolist()
    assert abs(st.loss - c["loss"]) <= GC.FP64_GATE * max(abs(c["loss"]), 1.0) and st.norm is None
    c = GC.load("grad_sm_clip")
    p = c["p"]
    sm = SoftmaxStepper(c["X"], c["y"], p["C"], engine=engine)
    delta = sm.private_fun(c["ww"], c["idx"])
    gate = GC.softmax_gate(p["din"], p["count"])
    scale = R.softmax_scale(c["X"], c["idx"])
    assert np.max(np.abs(delta - c["delta"])) <= gate * scale
    assert sm.norm > 100.0 and abs(sm.norm - c["norm"]) <= gate * max(c["norm"], scale)
