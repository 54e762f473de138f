"""The last arrival and the finish in one call (bk_collect_add_finish,
bk_collect_arrive.hip): the row's copy, then ONE launch -- k_collect_arrive, the
border of the new row in front of k_collect_small's work items.

The bar: collect_stats() and the timing table show the path taken; every output
-- sel, scores, mean and the eight margin fields -- is BITWISE what
bk_collect_add followed by bk_collect_finish gives on the same engine after a
fresh bk_collect_begin with the same rows (the reference of every check here,
never the fused call itself), and so is everything a later add or finish sees."""
import ctypes

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import Engine, KRUMValidator, Update  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"
FUSED = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 1}
TWO_SMALL = {"border": 1, "border_reduce": 1, "one_launch_finishes": 1, "fused_arrivals": 0}
TWO_CHAIN = {"border": 1, "border_reduce": 1, "one_launch_finishes": 0, "fused_arrivals": 0}


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


def _begin(engine, X, upto, n_cap=None, group=30):
    """a fresh collection holding rows 0..upto-1 of X"""
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


def _two_calls(engine, X, j, n_cap=None, **kw):
    """THE REFERENCE: rows 0..j-1 collected afresh, then collect_add(X[j]) and
    collect_finish(**kw) -> ((sel, scores, mean), record), the launches taken"""
    _begin(engine, X, j, n_cap)
    s0 = engine.collect_stats()
    assert engine.collect_add(X[j]) == j
    out = _finish(engine, **kw)
    return out, _delta(engine.collect_stats(), s0)


def _arrive(engine, row, **kw):
    """collect_add_finish from pageable memory -- or, past the 32 KiB where a
    pageable row takes the two calls inside the entry, from pinned memory, so
    that the fused launch is what runs"""
    if row.nbytes <= 32768:
        return engine.collect_add_finish(row, **kw)
    t = torch.from_numpy(np.ascontiguousarray(row)).pin_memory()
    return engine.collect_add_finish(t.numpy(), where=_lib.BK_HOST_PINNED, **kw)


def _fused(engine, X, j, n_cap=None, **kw):
    """rows 0..j-1 collected afresh, then collect_add_finish(X[j], **kw)"""
    _begin(engine, X, j, n_cap)
    s0 = engine.collect_stats()
    slot, sel, sc, mean = _arrive(engine, X[j], **kw)
    assert slot == j and engine.collect_count() == j + 1
    return ((sel, sc, mean), _record(engine)), _delta(engine.collect_stats(), s0)


def _both(engine, X, what, path=FUSED, n_cap=None, **kw):
    """the fused call against the reference, bitwise, on the expected path"""
    j = X.shape[0] - 1
    ref, rs = _two_calls(engine, X, j, n_cap, **kw)
    got, gs = _fused(engine, X, j, n_cap, **kw)
    if path is not FUSED and X[j].nbytes > 32768:  # pinned there; the same from pageable memory
        _begin(engine, X, j, n_cap)
        slot, sel, sc, mean = engine.collect_add_finish(X[j], **kw)
        _assert_bitwise(((sel, sc, mean), _record(engine)), ref, (what, "pageable"))
    assert gs == path, (what, gs)
    _assert_bitwise(got, ref, what)
    return got, ref, rs


def test_path_taken(engine, oracle):
    """Fails without the feature: at (20, 200, f = 6) with 19 rows added, one
    more fused launch and no more border launches; the timing table shows
    k_small once and none of the chain's kernels."""
    X = oracle.synth(20, 200, 41, 3)
    ref, rs = _two_calls(engine, X, 19, f=6)
    assert rs == TWO_SMALL, rs
    _begin(engine, X, 19)
    s0 = engine.collect_stats()
    assert s0["fused_arrivals"] == 0 and s0["border"] == s0["border_reduce"] == 3  # 19 rows by 8
    engine.timing_enable(True)
    slot, sel, sc, mean = engine.collect_add_finish(X[19], f=6)
    t = engine.timing_read()
    engine.timing_enable(False)
    assert slot == 19
    assert _delta(engine.collect_stats(), s0) == FUSED
    assert ONE in t and t[ONE]["count"] == 1, t
    assert not any(k in t for k in CHAIN + ("k_mean", "d2h", "h2d")), t
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref, "fused")
    # the small path off: the border and the chain, the same bits
    engine.set_small_path(False)
    try:
        _begin(engine, X, 19)
        s0 = engine.collect_stats()
        engine.timing_enable(True)
        slot, sel, sc, mean = engine.collect_add_finish(X[19], f=6)
        t = engine.timing_read()
        engine.timing_enable(False)
        off = ((sel, sc, mean), _record(engine))
    finally:
        engine.set_small_path(True)
    assert _delta(engine.collect_stats(), s0) == TWO_CHAIN
    assert ONE not in t and all(k in t for k in CHAIN), t
    _assert_bitwise(off, ref, "small path off")


@pytest.mark.parametrize("n,d,f,dtype", [
    (2, 1, 1, np.float64), (2, 25, 1, np.float64), (16, 25, 5, np.float64),
    (17, 1023, 5, np.float64), (33, 1024, 10, np.float64), (64, 1025, 20, np.float64),
    (100, 7850, 30, np.float64), (127, 333, 40, np.float64), (128, 32768, 38, np.float64),
    (2, 1, 1, np.float32), (16, 25, 5, np.float32), (17, 2047, 5, np.float32),
    (65, 2048, 20, np.float32), (90, 2049, 30, np.float32), (100, 7850, 30, np.float32),
    (128, 32768, 38, np.float32)])
def test_bitwise_against_add_then_finish(engine, oracle, n, d, f, dtype):
    """every NB = ceil(n / 16) instantiation, one resident row, d on both sides of
    the chunk boundaries (1,024 fp64 / 2,048 fp32 columns), one chunk to 32"""
    X = oracle.synth(n, d, 700 + n + d, max(1, f // 2), dtype=dtype)
    got, _, rs = _both(engine, X, (n, d, f), f=f)
    assert rs == TWO_SMALL, rs
    assert int(got[1][6]) == d and int(got[1][7]) == max(0, n - f - 2)


def test_row_sources(engine, oracle):
    """an odd d with pageable rows off 16-byte alignment; pinned and device rows"""
    n, d, f = 37, 1003, 11
    X = oracle.synth(n, d, 71, 5)
    ref, _ = _two_calls(engine, X, n - 1, f=f)
    buf = np.empty(n * d + 1, dtype=np.float64)
    rows = buf[1:].reshape(n, d)  # row i starts 8 (i d + 1) bytes in: 8 mod 16 for even i
    rows[:] = X
    assert rows[n - 1].ctypes.data % 16 == 8
    got, gs = _fused(engine, rows, n - 1, f=f)
    assert gs == FUSED
    _assert_bitwise(got, ref, "unaligned pageable")
    last = torch.from_numpy(np.ascontiguousarray(X[n - 1]))
    for where, t in ((_lib.BK_HOST_PINNED, last.pin_memory()), (_lib.BK_DEVICE, last.cuda())):
        torch.cuda.synchronize()
        _begin(engine, X, n - 1)
        sel, sc, mean = np.empty(n - f, np.int64), np.empty(n), np.empty(d)
        slot, m = engine.collect_add_finish_ptr(t.data_ptr(), where, None, n, f, sel.ctypes.data,
                                                sc.ctypes.data, mean.ctypes.data)
        assert (slot, m) == (n - 1, n - f)
        assert engine.collect_stats()["fused_arrivals"] == 1
        _assert_bitwise(((sel, sc, mean), _record(engine)), ref, where)


def test_orders(engine, oracle):
    n, d, f = 60, 777, 18
    X = oracle.synth(n, d, 72, 9)
    rng = np.random.default_rng(8)
    perm = rng.permutation(n).astype(np.int64)
    with_new = np.concatenate([rng.choice(n - 1, size=20, replace=False), [n - 1]]).astype(np.int64)
    rng.shuffle(with_new)
    without = rng.choice(n - 1, size=21, replace=False).astype(np.int64)
    _both(engine, X, "null order", f=f)
    _both(engine, X, "permutation", order=perm, f=f)
    _both(engine, X, "subset with the new slot", order=with_new, f=6)
    _both(engine, X, "subset without the new slot", order=without, f=6)
    # ... whose border was written all the same: a finish over every row
    after = _finish(engine, f=f)
    _two_calls(engine, X, n - 1, order=without, f=6)
    _assert_bitwise(after, _finish(engine, f=f), "all rows after the subset")
    # 70 rows of a 128-row collection
    Y = oracle.synth(128, 96, 73, 30)
    sub = np.concatenate([rng.choice(127, size=69, replace=False), [127]]).astype(np.int64)
    rng.shuffle(sub)
    _both(engine, Y, "70 of 128", order=sub, f=21)


def _history(engine, X, j, fused, f):
    """rows 0..j-1, then the arrival of row j with its finish, fused or not"""
    if fused:
        return _fused(engine, X, j, n_cap=X.shape[0], f=f)[0]
    return _two_calls(engine, X, j, n_cap=X.shape[0], f=f)[0]


def _later(engine, X, j):
    """what later calls see of a collection whose row j arrived: a finish on the
    one-launch path and on the chain, batched and ragged finishes over the new
    slot, then a plain add and a finish, and two more arrivals with their verdicts"""
    n = X.shape[0]
    out = []
    out.append(_finish(engine, f=j // 3))
    engine.set_small_path(False)
    try:
        out.append(_finish(engine, f=j // 3))
    finally:
        engine.set_small_path(True)
    rng = np.random.default_rng(j)
    orders = np.stack([np.concatenate([rng.choice(j, size=11, replace=False), [j]])
                       for _ in range(3)]).astype(np.int64)
    out.append(engine.collect_finish_batch(orders, 4))
    ragged = [np.arange(j + 1, dtype=np.int64)[::-1].copy(), orders[0][:5].copy(),
              np.array([j, 0, 3], dtype=np.int64)]
    out.append(engine.collect_finish_ragged(ragged, [j // 2, 2, 1]))
    assert engine.collect_add(X[j + 1]) == j + 1
    out.append(_finish(engine, f=j // 3))
    return out, n


def _same_later(a, b):
    for q in (0, 1, 4):
        _assert_bitwise(a[q], b[q], ("later", q))
    for q in (2, 3):
        (asel, asc, am), (bsel, bsc, bm) = a[q], b[q]
        assert all(np.array_equal(x, y) for x, y in zip(asel, bsel)), q
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(asc, bsc)), q
        assert np.array_equal(_bits(am), _bits(bm)), q


def test_state_afterwards(engine, oracle):
    n, d, j = 45, 1500, 40
    X = oracle.synth(n, d, 74, 12)
    _history(engine, X, j, False, 13)
    want, _ = _later(engine, X, j)
    want_more = []
    for r in (j + 2, j + 3):  # the verdict after each further arrival
        assert engine.collect_add(X[r]) == r
        want_more.append(_finish(engine, f=13))
    _history(engine, X, j, True, 13)
    got, _ = _later(engine, X, j)
    _same_later(got, want)
    for r, ref in zip((j + 2, j + 3), want_more):
        s0 = engine.collect_stats()
        slot, sel, sc, mean = engine.collect_add_finish(X[r], f=13)
        assert slot == r and _delta(engine.collect_stats(), s0) == FUSED
        _assert_bitwise(((sel, sc, mean), _record(engine)), ref, ("arrival", r))


def test_fallbacks_same_bits(engine, oracle):
    """outside the fused range the call is the add and then the finish"""
    # 129 rows after the add; a finish of 100 of them is the one-launch finish
    X = oracle.synth(129, 40, 75, 10)
    sub = np.concatenate([np.random.default_rng(2).choice(128, size=99, replace=False),
                          [128]]).astype(np.int64)
    _both(engine, X, "129 rows collected", path=TWO_SMALL, order=sub, f=30)
    _both(engine, X, "n = 129", path=TWO_CHAIN, f=40)
    # a pageable row of more than 32 KiB (measured no faster fused): the two calls
    W = oracle.synth(100, 7850, 80, 30)
    ref, _ = _two_calls(engine, W, 99, f=30)
    _begin(engine, W, 99)
    s0 = engine.collect_stats()
    slot, sel, sc, mean = engine.collect_add_finish(W[99], f=30)
    assert slot == 99 and _delta(engine.collect_stats(), s0) == TWO_SMALL
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref, "long pageable row")
    # d past k_collect_small's cap: the chain, or with the wide path on its launch
    Z = oracle.synth(5, 40000, 76, 1)
    _both(engine, Z, "d = 40,000", path=TWO_CHAIN, f=1)
    engine.set_collect_wide(True)
    try:
        _both(engine, Z, "d = 40,000, wide", path=TWO_SMALL, f=1)
    finally:
        engine.set_collect_wide(False)


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows", "edge_zeros_tie",
                                  "A_n4_k0_tie", "edge_k1", "half_clip"])
def test_special_values(name, engine, oracle):
    """the special row (where the case has one) arrives last: the finish's order
    puts the rows back in the golden's"""
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X)
    n = X.shape[0]
    bad = np.flatnonzero(~np.isfinite(X).all(axis=1))
    sp = int(bad[0]) if bad.size else n - 1
    arrive = np.array([r for r in range(n) if r != sp] + [sp], dtype=np.int64)
    order = np.empty(n, np.int64)
    order[arrive] = np.arange(n)  # the caller's row r sits at arrival slot order[r]
    A = np.ascontiguousarray(X[arrive])
    got, _, _ = _both(engine, A, name, order=order, f=p["f"])
    assert np.array_equal(got[0][0], GU.load(name)["sel"]), name


def test_interleaving(engine, oracle):
    """bk_multikrum's small host entry shares the queue lines and the mapped
    block: between two fused calls each result is its lone-call counterpart"""
    n, d, f = 100, 7850, 30
    X = oracle.synth(n, d, 77, 30)
    Y = oracle.synth(n, d, 78, 30)
    host_ref = engine.multikrum(Y, f)
    host_rec = _record(engine)
    _begin(engine, X, n - 2)
    assert engine.collect_add(X[n - 2]) == n - 2
    ref1 = _finish(engine, f=f)
    assert engine.collect_add(X[n - 1]) == n - 1
    ref2 = _finish(engine, f=f)
    _begin(engine, X, n - 2)
    _, sel, sc, mean = _arrive(engine, X[n - 2], f=f)
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref1, "first")
    got = engine.multikrum(Y, f)
    assert np.array_equal(got[0], host_ref[0])
    assert np.array_equal(_bits(got[1]), _bits(host_ref[1]))
    assert np.array_equal(_bits(got[2]), _bits(host_ref[2]))
    assert _same_record(_record(engine), host_rec)
    _, sel, sc, mean = _arrive(engine, X[n - 1], f=f)
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref2, "second")
    assert engine.collect_stats()["fused_arrivals"] == 2


def test_errors_leave_the_collection(engine, oracle):
    n, d, f = 12, 64, 3
    X = oracle.synth(n + 1, d, 79, 2)
    L = _lib.lib()
    sel = np.empty(n + 1, np.int64)
    row = np.ascontiguousarray(X[n])

    def call(ctx, rowp, where, order, nn, ff):
        o = np.ascontiguousarray(order, dtype=np.int64) if order is not None else None
        return L.bk_collect_add_finish(ctx, rowp, where, o.ctypes.data if o is not None else None,
                                       nn, ff, None, sel.ctypes.data, None, None, None)

    fresh = Engine(0)  # no begin on this context
    try:
        assert call(fresh.ctx, row.ctypes.data, _lib.BK_HOST, None, 2, 1) == _lib.BK_EINVAL
        assert "without bk_collect_begin" in _lib.last_error()
        # a first-ever arrival cannot finish: n = 1 leaves no f
        fresh.collect_begin(4, d)
        assert call(fresh.ctx, row.ctypes.data, _lib.BK_HOST, None, 1, 1) == _lib.BK_EINVAL
        assert call(fresh.ctx, row.ctypes.data, _lib.BK_HOST, None, 1, 0) == _lib.BK_EINVAL
        assert fresh.collect_count() == 0
    finally:
        fresh.close()

    _begin(engine, X, n, n_cap=n + 1)
    ref = _finish(engine, f=f)
    s0 = engine.collect_stats()
    bad = [
        (None, _lib.BK_HOST, None, n + 1, f, "null row"),
        (row.ctypes.data, 7, None, n + 1, f, "bad where"),
        (row.ctypes.data, _lib.BK_HOST, [0, 1, n + 1], 3, 1, "no collected slot"),
        (row.ctypes.data, _lib.BK_HOST, [-1, 1, 2], 3, 1, "no collected slot"),
        (row.ctypes.data, _lib.BK_HOST, [0, n, 0], 3, 1, "repeats a slot"),
        (row.ctypes.data, _lib.BK_HOST, None, n, f, "a null order needs"),
        (row.ctypes.data, _lib.BK_HOST, None, n + 2, f, "rows collected"),
        (row.ctypes.data, _lib.BK_HOST, None, n + 1, 0, "need 1 <= f < n"),
        (row.ctypes.data, _lib.BK_HOST, None, n + 1, n + 1, "need 1 <= f < n"),
    ]
    for rowp, where, order, nn, ff, word in bad:
        assert call(engine.ctx, rowp, where, order, nn, ff) == _lib.BK_EINVAL, word
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert engine.collect_count() == n
    assert L.bk_collect_add_finish(engine.ctx, row.ctypes.data, _lib.BK_HOST, None, n + 1, f, None,
                                   None, None, None, None) == _lib.BK_EINVAL
    assert "null sel_idx" in _lib.last_error()
    assert engine.collect_stats() == s0
    _assert_bitwise(_finish(engine, f=f), ref, "after the refused calls")
    # the new slot is a collected slot for the order: n names it
    slot, s, _, _ = engine.collect_add_finish(row, order=[n, 0, 5], f=1)
    assert slot == n and engine.collect_count() == n + 1
    # past n_cap
    assert call(engine.ctx, row.ctypes.data, _lib.BK_HOST, None, n + 2, f) == _lib.BK_EINVAL
    assert "past n_cap" in _lib.last_error()
    assert engine.collect_count() == n + 1


def _validators(engine, X, ids, arrival):
    n = len(ids)
    two = KRUMValidator(engine=engine, collect=True, n_cap=n).initialize()
    for i in arrival:
        two.add_update(Update(SourceID=ids[i], NoisedDelta=X[i]))
    two.compute_scores()
    one = KRUMValidator(engine=engine, collect=True, n_cap=n).initialize()
    for i in arrival[:-1]:
        one.add_update(Update(SourceID=ids[i], NoisedDelta=X[i]))
    s0 = engine.collect_stats()
    one.add_update(Update(SourceID=ids[arrival[-1]], NoisedDelta=X[arrival[-1]]), last=True)
    # (the validator's rows are pageable: fused up to 32 KiB a row)
    assert _delta(engine.collect_stats(), s0) == (FUSED if X[0].nbytes <= 32768 else TWO_SMALL)
    assert [u.SourceID for u in one.UpdateList] == sorted(ids)
    assert [u.SourceID for u in one.UpdateList] == [u.SourceID for u in two.UpdateList]
    assert all(np.array_equal(a.NoisedDelta, b.NoisedDelta)
               for a, b in zip(one.UpdateList, two.UpdateList))
    assert one.AcceptedList == two.AcceptedList
    return one


def test_krum_validator_last(engine, oracle):
    """add_update(..., last=True) is krum.go:291-314 in one call"""
    X, p = GU.build_input("B_mnist", oracle)
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    ids = [7 + 3 * i for i in range(n)]
    v = _validators(engine, X, ids, [int(i) for i in np.random.default_rng(4).permutation(n)])
    assert len(v.AcceptedList) == n - int(0.5 * n)
    T, _ = GU.build_input("A_n4_k0_tie", oracle)  # n = 4, f = 2: every score 0
    T = np.ascontiguousarray(T, dtype=np.float64)
    v = _validators(engine, T, [40, 10, 30, 20], [2, 0, 3, 1])
    assert len(v.AcceptedList) == 2
