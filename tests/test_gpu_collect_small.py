"""The one-launch finish of an incremental collection (k_collect_small,
bk_small.hip): for n <= 128 and d <= 32,768 bk_collect_finish is ONE launch --
k_small's S and M items reading the collection's arrival-slot Gram and row
store through the caller's order, which travels in the kernel arguments, the
outputs written into the context's mapped block (no upload before, no copy
after).  bk_set_small_path(ctx, 0) gives the chain (gather, K2, K3, K3b,
selmap, K4) on the same collection: the A/B these tests use.

The bar: the timing table shows the path taken; every output of the one-launch
finish -- sel, scores, mean and the eight margin fields -- is BITWISE the chain
finish's (both read the same Gram bits; the S items reproduce K2's summation
shape, the M items K4's adds); sel and mean bitwise bk_multikrum's on the rows
packed in the finish's order, scores within the collection's 1e-9 contract."""
import ctypes

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _record(engine):
    """the eight public margin fields of the last call, raw"""
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _same_record(a, b):
    """bitwise, a NaN matching a NaN"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _finish(engine, small, **kw):
    """collect_finish on the one-launch path (small) or the chain -> (outputs, record)"""
    engine.set_small_path(small)
    try:
        out = engine.collect_finish(**kw)
        return out, _record(engine)
    finally:
        engine.set_small_path(True)


def _timed_finish(engine, small, **kw):
    engine.set_small_path(small)
    try:
        engine.timing_enable(True)
        engine.collect_finish(**kw)
        t = engine.timing_read()
        engine.timing_enable(False)
        return t
    finally:
        engine.set_small_path(True)


def _collect(engine, X, group=30, n_cap=None):
    n, d = X.shape
    engine.collect_begin(n_cap or n, d, X.dtype)
    for i in range(0, n, group):
        assert engine.collect_add([X[r] for r in range(i, min(n, i + group))]) == i
    assert engine.collect_count() == n


def _assert_bitwise(got, ref, what):
    (gs, gsc, gm), grec = got
    (rs, rsc, rm), rrec = ref
    assert np.array_equal(gs, rs), (what, "sel", gs, rs)
    if gm is not None and rm is not None:
        assert np.array_equal(_bits(gm), _bits(rm)), (what, "mean")
    assert _same_record(grec, rrec), (what, "margin", grec, rrec)
    if gsc is not None and rsc is not None:
        diff = np.flatnonzero(_bits(gsc) != _bits(rsc))
        assert diff.size == 0, (what, "scores differ at rows", diff[:8], gsc[diff[:8]],
                                rsc[diff[:8]])


def _scores_close(sc, ref):
    """the collection's contract against the packed call: 1e-9 of the largest
    finite score, the same NaN / inf pattern"""
    assert np.array_equal(np.isnan(sc), np.isnan(ref))
    assert np.array_equal(np.isposinf(sc), np.isposinf(ref))
    fin = np.isfinite(ref)
    if fin.any():
        assert np.max(np.abs(sc[fin] - ref[fin])) <= 1e-9 * np.max(np.abs(ref[fin]))


def _on_off_and_packed(engine, X, f, order=None, what=""):
    """finish on both paths (bitwise), and against bk_multikrum on X[order]"""
    kw = dict(f=f) if order is None else dict(order=order, f=f)
    on = _finish(engine, True, **kw)
    off = _finish(engine, False, **kw)
    _assert_bitwise(on, off, what)
    P = X if order is None else np.ascontiguousarray(X[order])
    ps, psc, pm = engine.multikrum(P, f)
    assert np.array_equal(on[0][0], ps), (what, "sel vs packed")
    assert np.array_equal(_bits(on[0][2]), _bits(pm)), (what, "mean vs packed")
    _scores_close(on[0][1], psc)
    return on


def test_path_taken(engine, oracle):
    """Fails without the one-launch finish: the timing table of a finish at
    (20, 200, 6) shows k_small once and none of the chain's kernels."""
    X = oracle.synth(20, 200, 41, 3)
    _collect(engine, X)
    t = _timed_finish(engine, True, f=6)
    assert ONE in t and t[ONE]["count"] == 1, t
    assert not any(k in t for k in CHAIN + ("k_mean", "d2h", "h2d")), t
    t = _timed_finish(engine, False, f=6)
    assert ONE not in t and all(k in t for k in CHAIN), t
    # past the path's shapes the chain runs: n = 129, and d = 32,832 > 32,768
    Y = oracle.synth(129, 40, 42, 10)
    _collect(engine, Y)
    t = _timed_finish(engine, True, f=40)
    assert ONE not in t and all(k in t for k in CHAIN), t
    Z = oracle.synth(4, 32832, 43, 1)
    _collect(engine, Z)
    t = _timed_finish(engine, True, f=1)
    assert ONE not in t and all(k in t for k in CHAIN), t
    # n is the finish's n, not the rows collected: 70 slots of 200
    W = oracle.synth(200, 96, 44, 30)
    _collect(engine, W)
    sub = np.random.default_rng(5).choice(200, size=70, replace=False).astype(np.int64)
    t = _timed_finish(engine, True, order=sub, f=21)
    assert ONE in t and t[ONE]["count"] == 1 and not any(k in t for k in CHAIN), t
    t = _timed_finish(engine, True, f=60)  # all 200: the chain
    assert ONE not in t and all(k in t for k in CHAIN), t


@pytest.mark.parametrize("n,d,f,dtype", [
    (2, 1, 1, np.float64), (3, 7, 1, np.float64), (5, 64, 2, np.float64), (16, 8, 5, np.float64),
    (17, 1001, 5, np.float64), (64, 4096, 20, np.float64), (100, 7850, 30, np.float64),
    (100, 7850, 50, np.float64), (127, 333, 40, np.float64), (128, 32768, 38, np.float64),
    (33, 1003, 10, np.float32), (100, 7852, 30, np.float32)])
def test_bitwise_against_the_chain(engine, oracle, n, d, f, dtype):
    """the rows arrive in a random order and the finish's order puts them back,
    so the packed reference is X itself"""
    X = oracle.synth(n, d, 500 + n + d, max(1, f // 2), dtype=dtype)
    perm = np.random.default_rng(n + d).permutation(n)  # slot s holds row perm[s]
    _collect(engine, np.ascontiguousarray(X[perm]))
    order = np.empty(n, np.int64)
    order[perm] = np.arange(n)
    on = _finish(engine, True, order=order, f=f)
    off = _finish(engine, False, order=order, f=f)
    _assert_bitwise(on, off, (n, d, f))
    ps, psc, pm = engine.multikrum(X, f)
    assert np.array_equal(on[0][0], ps)
    assert np.array_equal(_bits(on[0][2]), _bits(pm))
    _scores_close(on[0][1], psc)
    assert int(on[1][6]) == d and int(on[1][7]) == max(0, n - f - 2)


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows", "edge_zeros_tie",
                                  "A_n4_k0_tie", "edge_k1", "half_clip"])
def test_special_values(name, engine, oracle):
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X)
    _collect(engine, X)
    on = _finish(engine, True, f=p["f"])
    off = _finish(engine, False, f=p["f"])
    _assert_bitwise(on, off, name)
    assert np.array_equal(on[0][0], GU.load(name)["sel"]), name


def test_order_and_large_slots(engine, oracle):
    """slot ids >= 128 in the 16-bit order, the triangular index at large slots"""
    X = oracle.synth(600, 64, 77, 90)
    _collect(engine, X, group=30, n_cap=600)
    rng = np.random.default_rng(13)
    order = rng.choice(600, size=128, replace=False).astype(np.int64)
    assert order.max() >= 128 and not np.array_equal(order, np.sort(order))
    big = _on_off_and_packed(engine, X, 40, order, "128 of 600")
    small = _on_off_and_packed(engine, X, 2, order[:7].copy(), "7 of 600")
    assert small[0][0].shape == (5,)
    with pytest.raises(ValueError):  # a NULL order needs n = the rows collected
        engine.collect_finish(n=128, f=40)
    assert engine.collect_count() == 600
    again = _finish(engine, True, order=order, f=40)
    _assert_bitwise(again, big, "after the refused finish")


def test_nullable_outputs(engine, oracle):
    n, d, f = 67, 1003, 20
    X = oracle.synth(n, d, 88, 10)
    _collect(engine, X)
    full = _finish(engine, True, f=f)
    for ws, wm in ((True, False), (False, True), (False, False)):
        t = _timed_finish(engine, True, f=f, want_scores=ws, want_mean=wm)
        assert t[ONE]["count"] == 1 and not any(k in t for k in CHAIN), t
        got = _finish(engine, True, f=f, want_scores=ws, want_mean=wm)
        assert (got[0][1] is None) == (not ws) and (got[0][2] is None) == (not wm)
        _assert_bitwise(got, full, (ws, wm))


def test_interleaving_and_repeat(engine, oracle):
    """the host entry shares the mapped output block and the queue words with
    the finish; every result is bitwise its lone-call counterpart and
    selection_margin() follows the last finish"""
    n, d, f = 100, 7850, 30
    X = oracle.synth(n + 5, d, 99, 30)
    Y = oracle.synth(n, d, 98, 30)
    host_ref = engine.multikrum(Y, f)
    host_rec = _record(engine)
    _collect(engine, X[:n], n_cap=n + 5)
    ref = _finish(engine, True, f=f)
    sub = np.array([93, 4, 57, 11, 70, 0, 38], dtype=np.int64)
    ref7 = _finish(engine, True, order=sub, f=2)
    assert int(ref[1][6]) == d and int(ref7[1][6]) == d

    _assert_bitwise(_finish(engine, True, f=f), ref, "first")
    got = engine.multikrum(Y, f)
    assert np.array_equal(got[0], host_ref[0])
    assert np.array_equal(_bits(got[1]), _bits(host_ref[1]))
    assert np.array_equal(_bits(got[2]), _bits(host_ref[2]))
    assert _same_record(_record(engine), host_rec)
    _assert_bitwise(_finish(engine, True, f=f), ref, "after the host call")
    assert engine.collect_add([X[n + i] for i in range(5)]) == n
    _on_off_and_packed(engine, X, f + 2, None, "105 rows")
    first = np.arange(n, dtype=np.int64)
    for r in range(30):
        if r % 2 == 0:
            _assert_bitwise(_finish(engine, True, order=first, f=f), ref, r)
        else:
            _assert_bitwise(_finish(engine, True, order=sub, f=2), ref7, r)
        assert engine.selection_margin()["d"] == d
