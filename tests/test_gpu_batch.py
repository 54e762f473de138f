"""bk_multikrum_batch*: B independent Multi-Krum problems of one shape in one
call (k_small_batch / k_tiny_batch, bk_small.hip; the loop of single calls
outside their range).

The bar: every output of problem b -- sel, scores, mean and the eight margin
fields -- is BITWISE what bk_multikrum_device gives on that problem alone on the
same engine (a NaN matches a NaN), and the selection is the oracle's wherever
the problem's record says near_tie = 0."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"
PAD = 777.25  # fills the gaps between rows and problems: never read


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    """bitwise, a NaN matching a NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return (a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and
            np.array_equal(_bits(a[~nan]), _bits(b[~nan])))


def _record(engine):
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _records(engine, B):
    rec = (ctypes.c_double * (8 * B))()
    _lib.check(_lib.lib().bk_selection_margin_batch(engine.ctx, rec, B))
    return np.array(list(rec), dtype=np.float64).reshape(B, 8)


def _problems(n, d, B, seed, dtype=np.float64):
    """B seeded problems that differ from each other: a common drift, a few
    far-off rows, the scales varying with the problem"""
    rng = np.random.default_rng(seed)
    P = np.empty((B, n, d), dtype=np.float64)
    for b in range(B):
        P[b] = 0.01 * (b + 1) * rng.standard_normal(d) + 1e-3 * rng.standard_normal((n, d))
        far = rng.choice(n, size=max(1, n // 4), replace=False)
        P[b, far] += 0.05 * rng.standard_normal((far.size, d))
    return P.astype(dtype)


class Dev:
    """the problems P (B, n, d) laid out in one device buffer: row stride ld,
    problem stride `stride`, the base `off` elements past the allocation"""

    def __init__(self, P, ld=None, stride=None, off=0):
        self.P = P
        self.B, self.n, self.d = P.shape
        self.ld = ld or self.d
        self.stride = stride or self.n * self.ld
        self.off = off
        self.es = P.itemsize
        self.dt = _lib.BK_F32 if P.dtype == np.float32 else _lib.BK_F64
        flat = np.full(off + (self.B - 1) * self.stride + (self.n - 1) * self.ld + self.d, PAD,
                       dtype=P.dtype)
        for b in range(self.B):
            for i in range(self.n):
                s = off + b * self.stride + i * self.ld
                flat[s:s + self.d] = P[b, i]
        self.buf = torch.from_numpy(flat).cuda()

    def ptr(self, b=0):
        return self.buf.data_ptr() + (self.off + b * self.stride) * self.es


def _outs(B, n, d, m):
    return (torch.full((B * m,), -7, dtype=torch.int64, device="cuda"),
            torch.full((B * n,), PAD, dtype=torch.float64, device="cuda"),
            torch.full((B * d,), PAD, dtype=torch.float64, device="cuda"))


def _singles(engine, D, f, B=None):
    """bk_multikrum_device on each problem alone -> sel (B, m), scores (B, n),
    mean (B, d), records (B, 8)"""
    B = B or D.B
    n, d, m = D.n, D.d, D.n - f
    sel, sc, mean = _outs(B, n, d, m)
    recs = np.empty((B, 8))
    for b in range(B):
        engine.multikrum_device_ptr(D.ptr(b), D.dt, n, d, D.ld, f, sel.data_ptr() + 8 * b * m,
                                    sc.data_ptr() + 8 * b * n, mean.data_ptr() + 8 * b * d)
        recs[b] = _record(engine)
    return (sel.cpu().numpy().reshape(B, m), sc.cpu().numpy().reshape(B, n),
            mean.cpu().numpy().reshape(B, d), recs)


def _batched(engine, D, f, B=None, want_scores=True, want_mean=True):
    B = B or D.B
    n, d, m = D.n, D.d, D.n - f
    sel, sc, mean = _outs(B, n, d, m)
    engine.multikrum_batch_device_ptr(D.ptr(0), D.dt, B, n, d, D.ld, D.stride, f, sel.data_ptr(),
                                      sc.data_ptr() if want_scores else None,
                                      mean.data_ptr() if want_mean else None)
    engine.synchronize()
    recs = _records(engine, B)
    return (sel.cpu().numpy().reshape(B, m),
            sc.cpu().numpy().reshape(B, n) if want_scores else None,
            mean.cpu().numpy().reshape(B, d) if want_mean else None, recs)


def _pick(recs):
    """the record bk_selection_margin* reports after a batched call"""
    near = np.flatnonzero(recs[:, 2] != 0)
    if near.size:
        return recs[near[0]]
    return recs[np.argmin(recs[:, 0] - recs[:, 1])]


def _assert_bitwise(got, ref, what, B=None):
    B = B or got[0].shape[0]
    assert got[0].shape[0] == B
    assert np.array_equal(got[0], ref[0][:B]), (what, "sel", got[0], ref[0][:B])
    if got[1] is not None:
        for b in range(B):
            assert _same(got[1][b], ref[1][b]), (what, "scores of problem", b)
    if got[2] is not None:
        for b in range(B):
            assert _same(got[2][b], ref[2][b]), (what, "mean of problem", b)
    for b in range(B):
        assert _same(got[3][b], ref[3][b]), (what, "margin of problem", b, got[3][b], ref[3][b])


def _assert_oracle(oracle, P, f, sel, recs, what):
    for b in range(sel.shape[0]):
        if recs[b, 2] == 0:
            assert np.array_equal(sel[b], oracle.krum(P[b], f, False, False)[0]), (what, b)


_REF = {}


def _reference(engine, key, make):
    """one layout and its single-call results per key, shared by the cases"""
    if key not in _REF:
        D, f = make()
        _REF[key] = (D, f, _singles(engine, D, f))
    return _REF[key]


SHAPES = [(2, 200, 200), (17, 129, 130), (33, 1003, 1003), (100, 1003, 1003), (128, 4097, 4098)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [1, 2, 3, 7])
@pytest.mark.parametrize("n,d,ld", SHAPES)
def test_small_batch_shapes(engine, oracle, n, d, ld, batch, dtype):
    """d = 129 is just past k_tiny; ld = 1003 forces the scalar-load form; 4097
    leaves a ragged last chunk (ld = 4098: the 16-B form)"""
    f = n // 2
    D, f, ref = _reference(engine, (n, d, ld, f, dtype), lambda: (
        Dev(_problems(n, d, 7, 1000 + n + d, dtype), ld=ld), f))
    got = _batched(engine, D, f, B=batch)
    _assert_bitwise(got, ref, (n, d, batch), B=batch)
    _assert_oracle(oracle, D.P, f, got[0], got[3], (n, d, batch))
    assert _same(_record(engine), _pick(got[3]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f", [1, 32])
def test_small_batch_f_extremes(engine, oracle, f, dtype):
    n, d = 33, 1003
    D, f, ref = _reference(engine, (n, d, 1003, f, dtype), lambda: (
        Dev(_problems(n, d, 7, 1000 + n + d, dtype), ld=1003), f))
    for batch in (2, 7):
        got = _batched(engine, D, f, B=batch)
        _assert_bitwise(got, ref, (f, batch), B=batch)
        _assert_oracle(oracle, D.P, f, got[0], got[3], (f, batch))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ld,gap,off", [(208, 64, 0), (200, 1, 0), (200, 0, 8)],
                         ids=["padded", "odd-stride", "base+8B"])
def test_strides(engine, oracle, ld, gap, off, dtype):
    """ld > d with stride > n ld; an odd stride with an even ld (the whole
    batch takes the scalar-load form); a base pointer 8 bytes past 16-B
    alignment"""
    n, d, f, B = 33, 200, 16, 5
    P = _problems(n, d, B, 31, dtype)
    D = Dev(P, ld=ld, stride=n * ld + gap, off=off // P.itemsize)
    assert D.ptr(0) % 16 == off
    ref = _singles(engine, D, f)
    got = _batched(engine, D, f)
    _assert_bitwise(got, ref, (ld, gap, off))
    _assert_oracle(oracle, P, f, got[0], got[3], (ld, gap, off))
    # ... and the same bits as the packed layout gives
    packed = _batched(engine, Dev(P), f)
    _assert_bitwise(packed, ref, "packed")


def _timed(engine, call):
    engine.timing_enable(True)
    try:
        out = call()
        return out, engine.timing_read()
    finally:
        engine.timing_enable(False)


def test_more_problems_than_one_launch_holds(engine, oracle):
    """BK_BATCH_WS_BYTES bounds a launch's partials: at (100, 1003) a problem
    needs 8 chunks x (112^2 + 112) doubles, so two problems' worth makes W = 2
    and a batch of 5 three launches"""
    n, d, f = 100, 1003, 50
    D, f, ref = _reference(engine, (n, d, 1003, f, np.float64), lambda: (
        Dev(_problems(n, d, 7, 1000 + n + d, np.float64), ld=1003), f))
    per = 8 * (112 * 112 + 112) * 8
    os.environ["BK_BATCH_WS_BYTES"] = str(2 * per + per // 2)
    try:
        got, t = _timed(engine, lambda: _batched(engine, D, f, B=5))
    finally:
        del os.environ["BK_BATCH_WS_BYTES"]
    assert t[ONE]["count"] == 3 and not any(k in t for k in CHAIN), t
    _assert_bitwise(got, ref, "W = 2", B=5)
    _assert_oracle(oracle, D.P, f, got[0], got[3], "W = 2")
    got, t = _timed(engine, lambda: _batched(engine, D, f, B=7))
    assert t[ONE]["count"] == 1 and not any(k in t for k in CHAIN), t
    _assert_bitwise(got, ref, "one launch", B=7)
    # the A/B: the loop of single calls on the general chain
    engine.set_small_path(False)
    try:
        got, t = _timed(engine, lambda: _batched(engine, D, f, B=7))
        assert ONE not in t and all(t[k]["count"] == 7 for k in CHAIN), t
        chain = _singles(engine, D, f)
    finally:
        engine.set_small_path(True)
    _assert_bitwise(got, chain, "loop on the chain", B=7)
    clear = (got[3][:, 2] == 0) & (ref[3][:, 2] == 0)
    assert np.array_equal(got[0][clear], ref[0][clear])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,f", [(10, 25, 5), (16, 128, 8)])
def test_tiny_batch(engine, oracle, n, d, f, dtype):
    """k_tiny_batch: one workgroup per problem; 300 exceeds the CU count"""
    D = Dev(_problems(n, d, 300, 50 + n, dtype))
    ref = _singles(engine, D, f)
    for batch in (1, 5, 300):
        got, t = _timed(engine, lambda: _batched(engine, D, f, B=batch))
        assert t[ONE]["count"] == 1, t
        _assert_bitwise(got, ref, (n, d, batch), B=batch)
        _assert_oracle(oracle, D.P, f, got[0], got[3], (n, d, batch))
        assert _same(_record(engine), _pick(got[3]))


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows", "edge_zeros_tie",
                                  "edge_n2_f1", "A_n4_k0_tie"])
def test_isolation(name, engine, oracle):
    """a special-value golden as problem 2 of four: its neighbours are
    untouched, it is bitwise its single call and selects what the golden does"""
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X)
    n, d = X.shape
    f = p["f"]
    P = _problems(n, d, 4, 7 + n + d, X.dtype)
    P[2] = X
    D = Dev(P)
    ref = _singles(engine, D, f)
    got = _batched(engine, D, f)
    _assert_bitwise(got, ref, name)
    assert np.array_equal(got[0][2], GU.load(name)["sel"]), name
    _assert_oracle(oracle, P[[0, 1, 3]], f, got[0][[0, 1, 3]], got[3][[0, 1, 3]], name)
    assert _same(_record(engine), _pick(got[3])), name
    if got[3][2, 2] != 0 and not (got[3][:2, 2] != 0).any():
        assert _same(_record(engine), got[3][2]), name


def test_nullable_outputs(engine, oracle):
    n, d, f = 33, 1003, 10
    D = Dev(_problems(n, d, 3, 61))
    full = _batched(engine, D, f)
    for ws, wm in ((True, False), (False, True), (False, False)):
        got = _batched(engine, D, f, want_scores=ws, want_mean=wm)
        assert (got[1] is None) == (not ws) and (got[2] is None) == (not wm)
        _assert_bitwise(got, full, (ws, wm))


def test_interleaving(engine, oracle):
    """a batched call, a single call, a collection finish and the batched call
    again on one context: separate queue lines and partials"""
    n, d, f = 100, 1003, 30
    D = Dev(_problems(n, d, 4, 71))
    Y = Dev(_problems(n, d, 1, 72))
    Z = oracle.synth(20, 200, 41, 3)
    engine.collect_begin(20, 200, Z.dtype)
    engine.collect_add([Z[r] for r in range(20)])
    alone_single = _singles(engine, Y, f)
    alone_finish = engine.collect_finish(f=6)
    alone_rec = _record(engine)

    first = _batched(engine, D, f)
    _assert_bitwise(_singles(engine, Y, f), alone_single, "single after batched")
    fin = engine.collect_finish(f=6)
    assert np.array_equal(fin[0], alone_finish[0])
    assert _same(fin[1], alone_finish[1]) and _same(fin[2], alone_finish[2])
    assert _same(_record(engine), alone_rec)
    with pytest.raises(ValueError):  # the last call is not a batched one
        _records(engine, 4)
    again = _batched(engine, D, f)
    _assert_bitwise(again, first, "batched again")
    _assert_bitwise(first, _singles(engine, D, f), "batched vs singles")


def test_host_entry_and_python(engine, oracle):
    n, d, f, B = 100, 1003, 50, 3
    P = _problems(n, d, B, 81)
    dev = _batched(engine, Dev(P), f)
    pinned = torch.from_numpy(P).pin_memory().numpy()
    for X, pin in ((P, False), (pinned, True)):
        sel, sc, mean = engine.multikrum_batch(X, f, pinned=pin)
        assert sel.shape == (B, n - f) and sel.dtype == np.int64
        assert sc.shape == (B, n) and sc.dtype == np.float64
        assert mean.shape == (B, d) and mean.dtype == np.float64
        recs = np.array([[r[k] for k in ("gap", "err_bound", "near_tie", "M", "s_lo", "s_hi",
                                         "d", "k")] for r in engine.selection_margin_batch(B)],
                        dtype=np.float64)
        _assert_bitwise((sel, sc, mean, recs), dev, ("host", pin))
    # uniform strides: every other row of a wider array, no copy needed
    wide = np.full((B, 2 * n, d + 5), PAD)
    wide[:, ::2, :d] = P
    sel, sc, mean = engine.multikrum_batch(wide[:, ::2, :d], f)
    _assert_bitwise((sel, sc, mean, _records(engine, B)), dev, "strided view")
    sel, sc, mean = engine.multikrum_batch(P, f, want_scores=False, want_mean=False)
    assert sc is None and mean is None and np.array_equal(sel, dev[0])
    from biscotti_amd import krum_batch
    ks = krum_batch([[list(map(float, row)) for row in prob] for prob in P[:, :12, :40]], 5,
                    engine=engine)
    assert ks.shape == (B, 7) and ks.dtype == np.int64
    for b in range(B):
        one = engine.multikrum(np.ascontiguousarray(P[b, :12, :40]), 5, False, False)[0]
        assert np.array_equal(ks[b], one)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fallback_loop(engine, oracle, dtype):
    """n = 129 is outside the one-launch range: the entry is a loop of the
    single-problem device path, bitwise three single calls"""
    n, d, f, B = 129, 64, 40, 3
    D = Dev(_problems(n, d, B, 91, dtype))
    ref = _singles(engine, D, f)
    got, t = _timed(engine, lambda: _batched(engine, D, f))
    assert ONE not in t and all(t[k]["count"] == B for k in CHAIN), t
    _assert_bitwise(got, ref, "loop")
    _assert_oracle(oracle, D.P, f, got[0], got[3], "loop")
    assert _same(_record(engine), _pick(got[3]))
