"""The last arrival of a WIDE row and its finish in one launch
(bk_set_collect_wide_arrive, bk_collect_arrive_wide.hip): with the wide path and
the switch on, bk_collect_add_finish of a pinned or a device row whose finish is
in the wide one-launch range is the row's copy and ONE launch --
k_collect_arrive_wide, the border of the new row spread over the grid in front of
k_collect_wide's items.

The bar: collect_stats() shows the path taken; every output -- sel, scores, mean
and the margin record -- is BITWISE what the existing route gives on the same
engine with the switch off: rows 0..j-1 collected afresh, then collect_add(X[j])
and collect_finish(...) (the reference of every check here, never the fused call
itself), and so is everything a later add or finish sees.

Each shape is the smallest at which one part of the kernel can go wrong:
  2 x 32,769 f64      33 chunks, one more than k_collect_arrive's LDS form holds;
                      the last chunk one column; the border i = 0 and the diagonal
  5 x 40,000 f64      the shape test_gpu_collect_arrive.py pins on the sequence
  17 x 66,001 f64     65 chunks: lane 0 of an R unit adds two; odd d; NB = 2
  128 x 32,776 f32    17 chunks of fp32 vectors; the 128-row cap
  100 x 163,850       the CNN shape, both dtypes, with and without the mean
  4 x 1,048,576 f64   1,024 chunks: 16 rounds per lane of an R unit"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import KRUMValidator, Update  # noqa: E402

ONE = "k_small"  # BK_K_SMALL: the fused launch is timed under it
CHAIN = ("k_scores", "k_rank", "k_compact")
FUSED = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 1}
TWO_SMALL = {"border": 1, "border_reduce": 1, "one_launch_finishes": 1, "fused_arrivals": 0}
TWO_CHAIN = {"border": 1, "border_reduce": 1, "one_launch_finishes": 0, "fused_arrivals": 0}
MEAN_MAX_D = 165888  # bk.h BK_COLLECT_WIDE_MEAN_MAX_D


@pytest.fixture
def wide(engine):
    """the engine with the wide path on; the new switch is set by each call"""
    engine.set_collect_wide(True)
    engine.set_collect_wide_arrive(False)
    yield engine
    engine.set_collect_wide_arrive(False)
    engine.set_collect_wide(False)


@functools.lru_cache(maxsize=None)
def _synth(oracle, n, d, seed, nbyz, dtype):
    X = oracle.synth(n, d, seed, nbyz, dtype=dtype)
    X.setflags(write=False)  # shared among the tests, unchanged
    return X


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _record(engine):
    """the last call's margin record, raw: the eight fields the ABI exposes of
    its nine words (the ninth, u_G, is write_margin's constant argument, 2^-53 on
    both routes: wide_rank_select writes the record in either)"""
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _same_record(a, b):
    """bitwise, a NaN matching a NaN"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _assert_bitwise(got, ref, what):
    (gs, gsc, gm), grec = got
    (rs, rsc, rm), rrec = ref
    assert np.array_equal(gs, rs), (what, "sel", gs, rs)
    assert (gm is None) == (rm is None) and (gsc is None) == (rsc is None), what
    if gm is not None:
        diff = np.flatnonzero(_bits(gm) != _bits(rm))
        assert diff.size == 0, (what, "mean differs at columns", diff[:8])
    assert _same_record(grec, rrec), (what, "margin", grec, rrec)
    if gsc is not None:
        diff = np.flatnonzero(_bits(gsc) != _bits(rsc))
        assert diff.size == 0, (what, "scores differ at rows", diff[:8], gsc[diff[:8]],
                                rsc[diff[:8]])


def _begin(engine, X, upto, n_cap=None, group=32):
    """a fresh collection holding rows 0..upto-1 of X, by plain adds"""
    n, d = X.shape
    engine.collect_begin(n_cap or n, d, X.dtype)
    for i in range(0, upto, group):
        assert engine.collect_add([X[r] for r in range(i, min(upto, i + group))]) == i
    assert engine.collect_count() == upto


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _finish(engine, **kw):
    out = engine.collect_finish(**kw)
    return out, _record(engine)


def _reference(engine, X, j, kws, n_cap=None):
    """THE REFERENCE, the switch off: rows 0..j-1 collected afresh, then
    collect_add(X[j]) and collect_finish(**kw) for every kw of kws (a finish
    leaves the collection as it was) -> [((sel, scores, mean), record)]"""
    engine.set_collect_wide_arrive(False)
    _begin(engine, X, j, n_cap)
    assert engine.collect_add(X[j]) == j
    return [_finish(engine, **kw) for kw in kws]


def _pinned(row):
    return torch.from_numpy(np.array(row)).pin_memory()


def _arrive(engine, X, j, where=_lib.BK_HOST_PINNED, on=True, n_cap=None, **kw):
    """rows 0..j-1 collected afresh, then collect_add_finish(X[j], **kw) with the
    switch set to `on` (True: the whole range; 1: the routing that ships; False)
    -> ((sel, scores, mean), record), the launches taken"""
    _begin(engine, X, j, n_cap)
    t = None
    if where == _lib.BK_HOST:
        row = np.array(X[j])
    else:
        t = _pinned(X[j]) if where == _lib.BK_HOST_PINNED else torch.from_numpy(np.array(X[j])).cuda()
        torch.cuda.synchronize()
    # everywhere: the launch in the whole range, not only where it ships (on = 1)
    engine.set_collect_wide_arrive(bool(on), everywhere=on is True)
    s0 = engine.collect_stats()
    try:
        if t is None:
            slot, sel, sc, mean = engine.collect_add_finish(row, **kw)
        else:
            n, d = X.shape
            order = kw.get("order")
            nn = len(order) if order is not None else j + 1
            f = kw["f"]
            sel = np.empty(nn - f, np.int64)
            sc = np.empty(nn) if kw.get("want_scores", True) else None
            mean = np.empty(d) if kw.get("want_mean", True) else None
            o = np.ascontiguousarray(order, dtype=np.int64) if order is not None else None
            slot, m = engine.collect_add_finish_ptr(
                t.data_ptr(), where, o.ctypes.data if o is not None else None, nn, f,
                sel.ctypes.data, sc.ctypes.data if sc is not None else None,
                mean.ctypes.data if mean is not None else None)
            assert m == nn - f
    finally:
        engine.set_collect_wide_arrive(False)
    assert slot == j and engine.collect_count() == j + 1
    return ((sel, sc, mean), _record(engine)), _delta(engine.collect_stats(), s0)


def _both(engine, X, what, kws, path=FUSED, n_cap=None, **how):
    """the fused call against the reference, bitwise, on the expected path, for
    every finish of kws"""
    j = X.shape[0] - 1
    refs = _reference(engine, X, j, kws, n_cap)
    for kw, ref in zip(kws, refs):
        got, gs = _arrive(engine, X, j, n_cap=n_cap, **how, **kw)
        assert gs == path, (what, kw.keys(), gs)
        _assert_bitwise(got, ref, (what, sorted(kw)))
    return refs


def test_path_taken(wide, oracle):
    """Fails without the feature.  5 x 40,000, f = 1, the shape
    test_gpu_collect_arrive.py pins on the sequence: with the new switch on, one
    fused launch and no border launch; with it off, in the same test, the
    sequence still.  The timing table shows k_small once and no chain kernel."""
    X = _synth(oracle, 5, 40000, 76, 1, np.float64)
    (ref,) = _reference(wide, X, 4, [dict(f=1)])
    got, gs = _arrive(wide, X, 4, on=False, f=1)
    assert gs == TWO_SMALL, gs
    _assert_bitwise(got, ref, "switch off")
    _begin(wide, X, 4)
    t = _pinned(X[4])
    wide.set_collect_wide_arrive(True)
    s0 = wide.collect_stats()
    wide.timing_enable(True)
    slot, sel, sc, mean = wide.collect_add_finish(t.numpy(), f=1, where=_lib.BK_HOST_PINNED)
    tt = wide.timing_read()
    wide.timing_enable(False)
    assert slot == 4 and _delta(wide.collect_stats(), s0) == FUSED
    assert ONE in tt and tt[ONE]["count"] == 1, tt
    assert not any(k in tt for k in CHAIN + ("k_mean", "d2h", "h2d")), tt
    _assert_bitwise(((sel, sc, mean), _record(wide)), ref, "fused")


def test_shipped_routing(wide, oracle):
    """bk_set_collect_wide_arrive(ctx, 1) takes the fused launch only where it
    was measured ahead of the sequence: a pinned row of at most
    320,000 bytes in a call that asks for the mean.  The same bits either way."""
    X = _synth(oracle, 5, 40000, 76, 1, np.float64)
    refs = _reference(wide, X, 4, [dict(f=1), dict(f=1, want_mean=False)])
    for where, kw, ref, path in ((_lib.BK_HOST_PINNED, dict(f=1), refs[0], FUSED),
                                 (_lib.BK_HOST_PINNED, dict(f=1, want_mean=False), refs[1], TWO_SMALL),
                                 (_lib.BK_DEVICE, dict(f=1), refs[0], TWO_SMALL)):
        got, gs = _arrive(wide, X, 4, where=where, on=1, **kw)
        assert gs == path, (where, kw, gs)
        _assert_bitwise(got, ref, (where, sorted(kw)))
    Y = _synth(oracle, 17, 66001, 917, 2, np.float64)  # 528,008-byte rows
    (ref,) = _reference(wide, Y, 16, [dict(f=5)])
    got, gs = _arrive(wide, Y, 16, on=1, f=5)
    assert gs == TWO_SMALL, gs
    _assert_bitwise(got, ref, "a row past the cut")


def test_row_sources_and_switches(wide, oracle):
    """pinned and device rows are fused; a pageable row, the wide path off and
    the small path off take the sequence; the same bits everywhere"""
    X = _synth(oracle, 5, 40000, 76, 1, np.float64)
    (ref,) = _reference(wide, X, 4, [dict(f=1)])
    for where, path in ((_lib.BK_HOST_PINNED, FUSED), (_lib.BK_DEVICE, FUSED),
                        (_lib.BK_HOST, TWO_SMALL)):
        got, gs = _arrive(wide, X, 4, where=where, f=1)
        assert gs == path, (where, gs)
        _assert_bitwise(got, ref, where)
    wide.set_collect_wide(False)
    got, gs = _arrive(wide, X, 4, f=1)
    wide.set_collect_wide(True)
    assert gs == TWO_CHAIN, gs
    _assert_bitwise(got, ref, "the switch on, wide off")
    wide.set_small_path(False)
    try:
        got, gs = _arrive(wide, X, 4, f=1)
    finally:
        wide.set_small_path(True)
    assert gs == TWO_CHAIN, gs
    _assert_bitwise(got, ref, "the small path off")


@pytest.mark.parametrize("n,d,f,dtype", [(2, 32769, 1, np.float64), (17, 66001, 5, np.float64),
                                         (128, 32776, 38, np.float32)])
def test_bitwise_small_shapes(wide, oracle, n, d, f, dtype):
    X = _synth(oracle, n, d, 900 + n, max(1, f // 2), dtype)
    refs = _both(wide, X, (n, d), [dict(f=f), dict(f=f, want_mean=False)])
    assert int(refs[0][1][6]) == d


def test_the_128_row_cap(wide, oracle):
    """a 129th collected row takes the sequence, whatever the finish names"""
    X = _synth(oracle, 129, 32776, 901, 10, np.float32)
    sub = np.concatenate([np.random.default_rng(2).choice(128, size=99, replace=False),
                          [128]]).astype(np.int64)
    _both(wide, X, "129 rows collected", [dict(order=sub, f=30)], path=TWO_SMALL)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cnn_shape(wide, oracle, dtype):
    """100 x 163,850: with and without the mean; a subset and a permutation that
    do not end in slot j; a device row"""
    n, d, f = 100, 163850, 30
    X = _synth(oracle, n, d, 902, 20, dtype)
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).astype(np.int64)
    if perm[-1] == n - 1:
        perm[[0, -1]] = perm[[-1, 0]]
    sub = np.concatenate([rng.choice(n - 1, size=40, replace=False), [n - 1]]).astype(np.int64)
    sub[[3, -1]] = sub[[-1, 3]]
    without = rng.choice(n - 1, size=33, replace=False).astype(np.int64)
    kws = [dict(f=f), dict(f=f, want_mean=False), dict(order=perm, f=f),
           dict(order=sub, f=12, want_mean=False), dict(order=without, f=9, want_mean=False)]
    refs = _both(wide, X, ("cnn", dtype.__name__), kws)
    got, gs = _arrive(wide, X, n - 1, where=_lib.BK_DEVICE, f=f, want_mean=False)
    assert gs == FUSED
    _assert_bitwise(got, refs[1], "device row")


def test_widest(wide, oracle):
    """4 x 1,048,576: fused without the mean; with it (past
    BK_COLLECT_WIDE_MEAN_MAX_D) the sequence, with the same bits"""
    X = _synth(oracle, 4, 1048576, 903, 1, np.float64)
    assert X.shape[1] > MEAN_MAX_D
    _both(wide, X, "no mean", [dict(f=1, want_mean=False)])
    _both(wide, X, "mean", [dict(f=1)], path=TWO_CHAIN)


def _later(engine, X, j):
    """what later calls see of a collection whose row j arrived: the stored row,
    a finish, a plain add and a finish, and ragged finishes over prefixes"""
    out = [engine.collect_read_rows([j])[0], _finish(engine, f=j // 3)]
    assert engine.collect_add(X[j + 1]) == j + 1
    out.append(_finish(engine, f=j // 3))
    prefixes = [np.arange(q, dtype=np.int64) for q in (j + 2, j + 1, j, 3)]
    out.append(engine.collect_finish_ragged(prefixes, [j // 3, j // 3, 2, 1]))
    return out


def test_state_afterwards(wide, oracle):
    """run j of the Gram is right in every element, not only where this finish
    read it: the fused finish names 3 rows, the later ones all of them"""
    n, d, j = 19, 66001, 16
    X = _synth(oracle, n, d, 904, 4, np.float64)
    order = np.array([j, 0, 5], dtype=np.int64)
    wide.set_collect_wide_arrive(False)
    _begin(wide, X, j, n_cap=n)
    assert wide.collect_add(X[j]) == j
    _finish(wide, order=order, f=1)
    want = _later(wide, X, j)
    got0, gs = _arrive(wide, X, j, n_cap=n, order=order, f=1)
    assert gs == FUSED
    got = _later(wide, X, j)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[0], X[j])
    _assert_bitwise(got[1], want[1], "finish after")
    _assert_bitwise(got[2], want[2], "add and finish after")
    (asel, asc, am), (bsel, bsc, bm) = got[3], want[3]
    assert all(np.array_equal(x, y) for x, y in zip(asel, bsel))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(asc, bsc))
    assert np.array_equal(_bits(am), _bits(bm))


def test_errors_leave_the_collection(wide, oracle):
    n, d, f = 4, 40000, 1
    X = _synth(oracle, 5, d, 76, 1, np.float64)
    L = _lib.lib()
    sel = np.empty(n + 1, np.int64)
    t = _pinned(X[n])
    _begin(wide, X, n, n_cap=n + 1)
    ref = _finish(wide, f=f)
    wide.set_collect_wide_arrive(True)
    s0 = wide.collect_stats()

    def call(rowp, where, order, nn, ff):
        o = np.ascontiguousarray(order, dtype=np.int64) if order is not None else None
        return L.bk_collect_add_finish(wide.ctx, rowp, where, o.ctypes.data if o is not None else None,
                                       nn, ff, None, sel.ctypes.data, None, None, None)

    PIN = _lib.BK_HOST_PINNED
    bad = [
        (None, PIN, None, n + 1, f, "null row"),
        (t.data_ptr(), 7, None, n + 1, f, "bad where"),
        (t.data_ptr(), PIN, [0, 1, n + 1], 3, 1, "no collected slot"),
        (t.data_ptr(), PIN, [0, n, 0], 3, 1, "repeats a slot"),
        (t.data_ptr(), PIN, [n], 1, 1, "need"),          # n < 2
        (t.data_ptr(), PIN, None, n, f, "a null order needs"),
        (t.data_ptr(), PIN, None, n + 1, 0, "need 1 <= f < n"),
    ]
    for rowp, where, order, nn, ff, word in bad:
        assert call(rowp, where, order, nn, ff) == _lib.BK_EINVAL, word
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert wide.collect_count() == n
    assert wide.collect_stats() == s0
    wide.set_collect_wide_arrive(False)
    _assert_bitwise(_finish(wide, f=f), ref, "after the refused calls")


def test_krum_validator_last(wide, oracle):
    """KRUMValidator(collect=True, wide=True, wide_arrive=True).add_update(u,
    last=True): the verdicts of the validator without the switch.  The
    validator asks for no mean, which the shipped routing (test_shipped_routing)
    sends through the sequence: the stats show that path, from pinned staging"""
    X = _synth(oracle, 5, 40000, 76, 1, np.float64)
    ids = [40, 10, 50, 30, 20]
    arrival = [2, 0, 4, 1, 3]
    two = KRUMValidator(engine=wide, collect=True, n_cap=5, wide=True).initialize()
    for i in arrival[:-1]:
        two.add_update(Update(SourceID=ids[i], NoisedDelta=X[i]))
    s0 = wide.collect_stats()
    two.add_update(Update(SourceID=ids[arrival[-1]], NoisedDelta=X[arrival[-1]]), last=True)
    assert _delta(wide.collect_stats(), s0) == TWO_SMALL
    one = KRUMValidator(engine=wide, collect=True, n_cap=5, wide=True, wide_arrive=True).initialize()
    try:
        for i in arrival[:-1]:
            one.add_update(Update(SourceID=ids[i], NoisedDelta=X[i]))
        s0 = wide.collect_stats()
        one.add_update(Update(SourceID=ids[arrival[-1]], NoisedDelta=X[arrival[-1]]), last=True)
        assert _delta(wide.collect_stats(), s0) == TWO_SMALL
    finally:
        wide.set_collect_wide_arrive(False)
    assert [u.SourceID for u in one.UpdateList] == sorted(ids)
    assert [u.SourceID for u in one.UpdateList] == [u.SourceID for u in two.UpdateList]
    assert one.AcceptedList == two.AcceptedList and len(one.AcceptedList) == 5 - 2
