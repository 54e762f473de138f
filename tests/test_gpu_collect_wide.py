"""The one-launch collection finishes for wide rows (k_collect_wide and
k_collect_wide_ragged, bk_collect_wide.hip): with bk_set_collect_wide on, a
finish of n <= 128 rows with 32,768 < d <= BK_COLLECT_WIDE_MAX_D is ONE launch --
k_collect_small's S items and queue, and M items that each stream 2,048 columns
of the selected rows from the row store -- and the batched and ragged entries
share launches there too.  The switch is off by default; with it off, or with
bk_set_small_path(ctx, 0), the launch chain (gather, K2, K3, K3b, selmap, K4)
runs on the same collection: the A/B these tests use.

The bar: the timing table shows the path taken; every output of the wide
finish -- sel, scores, mean and the eight margin fields -- is BITWISE the chain
finish's, and every problem of a batched or ragged call bitwise the single
finish's.  Every comparison is exact equality of bits; no tolerance appears."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"  # BK_K_SMALL: the wide launches are timed under it
W = 2048  # columns per wide M item (bk_internal.h COLLECT_WIDE_COLS)

# d: odd (a pad column and a one-column tail item); a multiple of 64 past the
# cap; the issue's "one item width + 1" and "two item widths - 64" -- taken
# literally they lie below the cap, where k_collect_small runs whatever the
# switch says, so they are kept AND joined by the smallest d of the same form
# inside the wide range (a one-column tail item; a tail item 64 columns short)
DS = (32769, 32832, W + 1, 2 * W - 64, 17 * W + 1, 18 * W - 64)
# (n, f): k = 0 and every score ties; NB = 1 full; NB steps to 2; f = n / 2; n = 128
NFS = ((2, 1), (16, 5), (17, 5), (100, 50), (128, 38))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _record(engine):
    """the eight public margin fields of the last call, raw"""
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _records(engine, batch):
    rec = (ctypes.c_double * (8 * batch))()
    _lib.check(_lib.lib().bk_selection_margin_batch(engine.ctx, rec, batch))
    return np.array(list(rec), dtype=np.float64).reshape(batch, 8)


@pytest.fixture
def wide(engine):
    """the session's engine with the wide finish on; off again afterwards"""
    engine.set_collect_wide(True)
    yield engine
    engine.set_collect_wide(False)
    engine.set_small_path(True)


def _finish(engine, small, **kw):
    """collect_finish with the small path on (wide, when switched on) or on the
    chain -> (outputs, record)"""
    engine.set_small_path(small)
    try:
        out = engine.collect_finish(**kw)
        return out, _record(engine)
    finally:
        engine.set_small_path(True)


def _timed(engine, call, small=True):
    engine.set_small_path(small)
    engine.timing_enable(True)
    try:
        out = call()
        return out, engine.timing_read()
    finally:
        engine.timing_enable(False)
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
    assert np.array_equal(_bits(grec), _bits(rrec)), (what, "margin", grec, rrec)
    if gsc is not None and rsc is not None:
        diff = np.flatnonzero(_bits(gsc) != _bits(rsc))
        assert diff.size == 0, (what, "scores differ at rows", diff[:8])


def _one_not_chain(t, count=1):
    return (ONE in t and t[ONE]["count"] == count and
            not any(k in t for k in CHAIN + ("k_mean", "d2h", "h2d")))


def test_path_taken(wide, oracle):
    """Fails without the feature: with the switch on, the timing table of a
    finish at (4, 32,832, f = 1) shows k_small once and none of the chain's
    kernels nor a copy."""
    engine = wide
    X = oracle.synth(4, 32832, 43, 1)
    _collect(engine, X)
    _, t = _timed(engine, lambda: engine.collect_finish(f=1))
    assert _one_not_chain(t), t
    # small path off: the chain, whatever the wide switch says
    _, t = _timed(engine, lambda: engine.collect_finish(f=1), small=False)
    assert ONE not in t and all(k in t for k in CHAIN), t
    # wide off (the default): the chain
    engine.set_collect_wide(False)
    _, t = _timed(engine, lambda: engine.collect_finish(f=1))
    assert ONE not in t and all(k in t for k in CHAIN), t
    engine.set_collect_wide(True)
    # n = 129 stays on the chain, d = 200 on k_collect_small
    Y = oracle.synth(129, 40, 42, 10)
    _collect(engine, Y)
    _, t = _timed(engine, lambda: engine.collect_finish(f=40))
    assert ONE not in t and all(k in t for k in CHAIN), t
    Z = oracle.synth(129, 32832, 45, 10, dtype=np.float32)
    _collect(engine, Z)
    _, t = _timed(engine, lambda: engine.collect_finish(f=40))
    assert ONE not in t and all(k in t for k in CHAIN), t
    V = oracle.synth(20, 200, 41, 3)
    _collect(engine, V)
    _, t = _timed(engine, lambda: engine.collect_finish(f=6))
    assert _one_not_chain(t), t
    # past BK_COLLECT_WIDE_MEAN_MAX_D (81 items of 2,048 columns) only a finish
    # without a mean stays on the wide launch; the bits are the chain's either way
    U = oracle.synth(4, 81 * W + 2, 46, 1)
    _collect(engine, U)
    got, t = _timed(engine, lambda: (engine.collect_finish(f=1), _record(engine)))
    assert ONE not in t and all(k in t for k in CHAIN), t
    nomean, t = _timed(engine, lambda: (engine.collect_finish(f=1, want_mean=False),
                                        _record(engine)))
    assert _one_not_chain(t), t
    _assert_bitwise(nomean, got, "no mean past the mean cap")
    U = np.ascontiguousarray(U[:, :81 * W])
    _collect(engine, U)
    got, t = _timed(engine, lambda: (engine.collect_finish(f=1), _record(engine)))
    assert _one_not_chain(t), t
    _assert_bitwise(got, _finish(engine, False, f=1), "at the mean cap")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", DS)
def test_bitwise_against_the_chain(wide, oracle, d, dtype):
    """every (n, f) over one 128-row collection of this d: the caller's rows are
    a random subset of the slots in random order, so the packed reference is
    X[order]"""
    engine = wide
    X = oracle.synth(128, d, 700 + d, 20, dtype=dtype)
    _collect(engine, X)
    rng = np.random.default_rng(d)
    for n, f in NFS:
        order = rng.permutation(128)[:n].astype(np.int64)
        on, t = _timed(engine, lambda: (engine.collect_finish(order=order, f=f), _record(engine)))
        assert _one_not_chain(t), (n, f, t)
        off = _finish(engine, False, order=order, f=f)
        _assert_bitwise(on, off, (n, d, f))
        ps, _, pm = engine.multikrum(np.ascontiguousarray(X[order]), f)
        assert np.array_equal(on[0][0], ps), (n, d, f, "sel vs packed")
        assert np.array_equal(_bits(on[0][2]), _bits(pm)), (n, d, f, "mean vs packed")
        assert int(on[1][6]) == d and int(on[1][7]) == max(0, n - f - 2)
        if n == 2:
            assert not on[0][1].any() and np.array_equal(on[0][0], [0])


def test_order_handling(wide, oracle):
    """a permutation with its inverse; 70 slots of 200 that include slots >= 128;
    finish, add rows, finish again"""
    engine = wide
    d = 33000
    X = oracle.synth(200, d, 77, 40)
    perm = np.random.default_rng(3).permutation(190)  # slot s holds row perm[s]
    _collect(engine, np.ascontiguousarray(X[:190][perm]), n_cap=200)
    inv = np.empty(100, np.int64)
    where = np.empty(190, np.int64)
    where[perm] = np.arange(190)
    inv[:] = where[:100]  # the caller's row i = X[i] sits at slot where[i]
    on = _finish(engine, True, order=inv, f=30)
    _assert_bitwise(on, _finish(engine, False, order=inv, f=30), "inverse")
    ps, _, pm = engine.multikrum(np.ascontiguousarray(X[:100]), 30)
    assert np.array_equal(on[0][0], ps) and np.array_equal(_bits(on[0][2]), _bits(pm))
    sub = np.random.default_rng(5).choice(190, size=70, replace=False).astype(np.int64)
    assert sub.max() >= 128 and not np.array_equal(sub, np.sort(sub))
    first = _finish(engine, True, order=sub, f=21)
    _assert_bitwise(first, _finish(engine, False, order=sub, f=21), "70 of 190")
    assert engine.collect_add([X[190 + i] for i in range(10)]) == 190
    _assert_bitwise(_finish(engine, True, order=sub, f=21), first, "after the add")
    sub2 = np.concatenate([sub[:60], np.arange(190, 200)]).astype(np.int64)
    _assert_bitwise(_finish(engine, True, order=sub2, f=21),
                    _finish(engine, False, order=sub2, f=21), "with the new rows")


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows", "edge_zeros_tie",
                                  "A_n4_k0_tie", "edge_k1", "half_clip"])
def test_special_values(name, wide, oracle):
    """the goldens' rows in the first columns of otherwise-zero wide rows"""
    engine = wide
    S, p = GU.build_input(name, oracle)
    S = np.ascontiguousarray(S)
    X = np.zeros((S.shape[0], 32832), dtype=S.dtype)
    X[:, :S.shape[1]] = S
    _collect(engine, X)
    on, t = _timed(engine, lambda: (engine.collect_finish(f=p["f"]), _record(engine)))
    assert _one_not_chain(t), t
    off = _finish(engine, False, f=p["f"])
    _assert_bitwise(on, off, name)
    assert np.array_equal(np.isnan(on[0][2]), np.isnan(off[0][2]))
    assert np.array_equal(np.isinf(on[0][2]), np.isinf(off[0][2]))


def test_nullable_outputs(wide, oracle):
    engine = wide
    n, d, f = 67, 32769, 20
    X = oracle.synth(n, d, 88, 10)
    _collect(engine, X)
    full = _finish(engine, True, f=f)
    for ws, wm in ((True, False), (False, True), (False, False)):
        got, t = _timed(engine, lambda: (engine.collect_finish(f=f, want_scores=ws, want_mean=wm),
                                         _record(engine)))
        assert _one_not_chain(t), t
        assert (got[0][1] is None) == (not ws) and (got[0][2] is None) == (not wm)
        _assert_bitwise(got, full, (ws, wm))


def _loop(engine, orders, fs):
    out = []
    for o, f in zip(orders, fs):
        out.append((engine.collect_finish(order=np.ascontiguousarray(o, dtype=np.int64), f=int(f)),
                    _record(engine)))
    return out


def test_ragged(wide, oracle):
    """ONE ragged call at d = 33,000 over a 130-row collection: four NB groups
    of two or more (wide launches), an n = 129 problem (the chain) and the only
    problem of its group (the single wide finish).  Every problem is bitwise
    collect_finish's, the records come back in the caller's order."""
    engine = wide
    d = 33000
    X = oracle.synth(130, d, 91, 30)
    _collect(engine, X)
    ns = [5, 100, 17, 129, 128, 20, 50, 7, 30, 99, 120]
    fs = [2, 50, 5, 40, 38, 19, 20, 1, 10, 30, 60]
    rng = np.random.default_rng(17)
    orders = [rng.choice(130, size=n, replace=False).astype(np.int64) for n in ns]
    assert max(int(o.max()) for o in orders) >= 128
    ref = _loop(engine, orders, fs)
    (sels, scs, mean), t = _timed(engine, lambda: engine.collect_finish_ragged(orders, fs))
    recs = _records(engine, len(ns))
    # groups NB = 1 (5, 7), 2 (17, 20, 30), 7 (100, 99), 8 (128, 120); single: 50
    assert t[ONE]["count"] == 4 + 1, t
    assert all(t[k]["count"] == 1 for k in CHAIN), t  # the n = 129 problem
    for b, ((rs, rsc, rm), rrec) in enumerate(ref):
        assert np.array_equal(sels[b], rs), (b, "sel")
        assert np.array_equal(_bits(scs[b]), _bits(rsc)), (b, "scores")
        assert np.array_equal(_bits(mean[b]), _bits(rm)), (b, "mean")
        assert np.array_equal(_bits(recs[b]), _bits(rrec)), (b, "margin", recs[b], rrec)
    # without a mean every problem has one M item
    (sels2, scs2, mean2), t = _timed(
        engine, lambda: engine.collect_finish_ragged(orders, fs, want_mean=False))
    assert mean2 is None and t[ONE]["count"] == 5, t
    for b in range(len(ns)):
        assert np.array_equal(sels2[b], sels[b]) and np.array_equal(_bits(scs2[b]), _bits(scs[b]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_uniform_batch(wide, oracle, dtype):
    """5 problems of (20, 32,832): one launch, bitwise the loop; with the
    per-launch output bound at two and a half means, three launches and the
    same bits"""
    engine = wide
    n, d, f = 20, 32832, 6
    X = oracle.synth(40, d, 93, 8, dtype=dtype)
    _collect(engine, X)
    rng = np.random.default_rng(23)
    orders = np.stack([rng.choice(40, size=n, replace=False) for _ in range(5)]).astype(np.int64)
    ref = _loop(engine, orders, [f] * 5)

    def check(got, recs, what):
        sel, sc, mean = got
        for b, ((rs, rsc, rm), rrec) in enumerate(ref):
            assert np.array_equal(sel[b], rs), (what, b, "sel")
            assert np.array_equal(_bits(sc[b]), _bits(rsc)), (what, b, "scores")
            assert np.array_equal(_bits(mean[b]), _bits(rm)), (what, b, "mean")
            assert np.array_equal(_bits(recs[b]), _bits(rrec)), (what, b, "margin")

    got, t = _timed(engine, lambda: engine.collect_finish_batch(orders, f))
    assert t[ONE]["count"] == 1 and not any(k in t for k in CHAIN + ("k_mean",)), t
    check(got, _records(engine, 5), "one launch")
    os.environ["BK_COLLECT_WIDE_OUT_BYTES"] = str(2 * d * 8 + d * 4)
    try:
        got, t = _timed(engine, lambda: engine.collect_finish_batch(orders, f))
    finally:
        del os.environ["BK_COLLECT_WIDE_OUT_BYTES"]
    assert t[ONE]["count"] == 3 and not any(k in t for k in CHAIN + ("k_mean",)), t
    check(got, _records(engine, 5), "three launches")
    # wide off: the loop of chain finishes, the same bits
    engine.set_collect_wide(False)
    got, t = _timed(engine, lambda: engine.collect_finish_batch(orders, f))
    assert ONE not in t and t["k_scores"]["count"] == 5, t
    check(got, _records(engine, 5), "the chain")


def test_errors_leave_the_state(wide, oracle):
    """every BK_EINVAL of the three finish entries, hit with wide on, leaves the
    collection and the margin state as they were"""
    engine = wide
    L = _lib.lib()
    assert L.bk_set_collect_wide(None, 1) == _lib.BK_EINVAL and _lib.last_error()
    n, d, f = 30, 32832, 9
    X = oracle.synth(n, d, 95, 5)
    _collect(engine, X)
    ref = _finish(engine, True, f=f)
    rec = _record(engine)
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    sel = np.zeros(4 * n, dtype=np.int64)
    ok = np.arange(n, dtype=np.int64)
    ctx = engine.ctx
    P = lambda a: a.ctypes.data  # noqa: E731
    bad_order, dup = ok.copy(), ok.copy()
    bad_order[3], dup[4] = n, 5
    off2 = i64(0, n, 2 * n)
    two = np.concatenate([ok, ok])
    calls = [
        lambda: L.bk_collect_finish(ctx, None, n, f, None, None, None, None),       # null sel
        lambda: L.bk_collect_finish(ctx, P(ok), 0, f, P(sel), None, None, None),    # n < 1
        lambda: L.bk_collect_finish(ctx, P(ok), n + 1, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish(ctx, None, n - 1, f, P(sel), None, None, None),  # null order
        lambda: L.bk_collect_finish(ctx, P(ok), n, 0, P(sel), None, None, None),    # f
        lambda: L.bk_collect_finish(ctx, P(ok), n, n, P(sel), None, None, None),
        lambda: L.bk_collect_finish(ctx, P(bad_order), n, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish(ctx, P(dup), n, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, P(two), 0, n, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, None, 2, n, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, P(two), 2, n, f, None, None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, P(two), 2, n + 1, f, P(sel), None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, P(two), 2, n, n, P(sel), None, None, None),
        lambda: L.bk_collect_finish_batch(ctx, P(np.concatenate([ok, dup])), 2, n, f, P(sel), None,
                                          None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(off2), P(i64(f, f)), 0, P(sel), None,
                                           None, None),
        lambda: L.bk_collect_finish_ragged(ctx, None, P(off2), P(i64(f, f)), 2, P(sel), None, None,
                                           None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), None, P(i64(f, f)), 2, P(sel), None, None,
                                           None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(off2), None, 2, P(sel), None, None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(off2), P(i64(f, f)), 2, None, None, None,
                                           None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(i64(1, n, 2 * n)), P(i64(f, f)), 2,
                                           P(sel), None, None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(i64(0, n, n)), P(i64(f, f)), 2, P(sel),
                                           None, None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(two), P(off2), P(i64(f, n)), 2, P(sel), None,
                                           None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(np.concatenate([ok, bad_order])), P(off2),
                                           P(i64(f, f)), 2, P(sel), None, None, None),
        lambda: L.bk_collect_finish_ragged(ctx, P(np.concatenate([dup, ok])), P(off2), P(i64(f, f)),
                                           2, P(sel), None, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == _lib.BK_EINVAL, (i, _lib.last_error())
        assert _lib.last_error()
        assert engine.collect_count() == n, i
        assert np.array_equal(_bits(_record(engine)), _bits(rec)), (i, "margin state")
    _assert_bitwise(_finish(engine, True, f=f), ref, "after the refused calls")
