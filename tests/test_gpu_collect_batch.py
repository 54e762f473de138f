"""bk_collect_finish_batch (k_collect_small_batch, bk_collect_batch.hip): many
finishes over ONE collection in one launch -- k_collect_small's S and M items
behind a problem index, each problem reading the collection's Gram and row
store through its own order.

The bar, in every case: each problem's sel, scores, mean and all eight margin
fields are BITWISE what a loop of bk_collect_finish gives on the same context
and collection (the same item bodies run on the same Gram bits).  Nothing is
tolerance-compared and nothing is skipped."""
import ctypes

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

ONE = "k_small"  # BK_K_SMALL as bk_timing_read names it: the batched launches are timed under it
CHAIN = ("k_scores", "k_rank", "k_compact")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    """bitwise, a NaN matching a NaN of any payload"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _record(engine):
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _records(engine, batch):
    rec = (ctypes.c_double * (8 * batch))()
    _lib.check(_lib.lib().bk_selection_margin_batch(engine.ctx, rec, batch))
    return np.array(list(rec), dtype=np.float64).reshape(batch, 8)


def _collect(engine, X, group=30, n_cap=None):
    n, d = X.shape
    engine.collect_begin(n_cap or n, d, X.dtype)
    for i in range(0, n, group):
        assert engine.collect_add([X[r] for r in range(i, min(n, i + group))]) == i
    assert engine.collect_count() == n


def _loop(engine, orders, f, ws=True, wm=True):
    """the parent's only equivalent: one bk_collect_finish per problem"""
    out = []
    for o in orders:
        sel, sc, mean = engine.collect_finish(order=np.ascontiguousarray(o, dtype=np.int64), f=f,
                                              want_scores=ws, want_mean=wm)
        out.append((sel, sc, mean, _record(engine)))
    return out


def _batch(engine, orders, f, ws=True, wm=True):
    orders = np.asarray(orders)
    sel, sc, mean = engine.collect_finish_batch(orders, f, want_scores=ws, want_mean=wm)
    B = orders.shape[0]
    return sel, sc, mean, _records(engine, B)


def _assert_same(got, ref, what):
    sel, sc, mean, recs = got
    assert sel.shape[0] == len(ref) == recs.shape[0], what
    for b, (rs, rsc, rm, rrec) in enumerate(ref):
        assert np.array_equal(sel[b], rs), (what, b, "sel", sel[b], rs)
        if sc is not None and rsc is not None:
            assert np.array_equal(np.isnan(sc[b]), np.isnan(rsc)), (what, b, "scores NaN")
            diff = np.flatnonzero(~np.isnan(rsc) & (_bits(sc[b]) != _bits(rsc)))
            assert diff.size == 0, (what, b, "scores differ at rows", diff[:8])
        if mean is not None and rm is not None:
            assert _same_bits(mean[b], rm), (what, b, "mean")
        assert _same_bits(recs[b], rrec), (what, b, "margin", recs[b], rrec)


def _timed(engine, call):
    engine.timing_enable(True)
    try:
        out = call()
        return out, engine.timing_read()
    finally:
        engine.timing_enable(False)


def _draw(rng, count, batch, n):
    """random subsets in random order: slots >= 128 occur once count > 128"""
    return np.stack([rng.choice(count, size=n, replace=False) for _ in range(batch)]).astype(np.int64)


# one 300-row collection per (d, dtype), shared by the cases that only read it
_ROWS = {}


def _rows(oracle, d, dtype):
    key = (d, np.dtype(dtype).name)
    if key not in _ROWS:
        X = oracle.synth(300, d, 9000 + d, 60, dtype=dtype)
        X.setflags(write=False)
        _ROWS[key] = X
    return _ROWS[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 25, 64, 65, 7850])
def test_bitwise_against_the_loop(engine, oracle, d, dtype):
    """Fails without the feature.  n over the NB boundaries and both ends of the
    range, d over one M item, the 64-column boundaries and more items than CUs,
    f = 1 and f = n - 1 (n = 3, f = 1: k = 0, every score 0, the tie rule
    decides), batches 1 (the single finish), 2, 3 and 7; random subsets and
    permutations of a 300-row collection"""
    X = _rows(oracle, d, dtype)
    _collect(engine, X)
    rng = np.random.default_rng(1000 + d)
    seen_big_slot = False
    for n in (3, 16, 17, 100, 128):
        for f in (1, n - 1):
            for batch in (1, 2, 3, 7):
                orders = _draw(rng, 300, batch, n)
                seen_big_slot |= bool(orders.max() >= 128)
                got, t = _timed(engine, lambda: _batch(engine, orders, f))
                assert t[ONE]["count"] == 1 and not any(k in t for k in CHAIN), (n, f, batch, t)
                assert got[0].shape == (batch, n - f) and got[1].shape == (batch, n)
                assert got[2].shape == (batch, d)
                _assert_same(got, _loop(engine, orders, f), (n, d, f, batch))
                if n == 3 and f == 1:
                    assert not got[1].any() and np.array_equal(got[0], [[0, 1]] * batch)
    assert seen_big_slot


def test_two_launches_past_1024_problems(engine, oracle):
    """1,025 problems at n = 10, d = 25: launches of at most 1,024 problems,
    so two of them, shown by the timing table"""
    X = _rows(oracle, 25, np.float64)
    _collect(engine, X)
    orders = _draw(np.random.default_rng(7), 300, 1025, 10)
    got, t = _timed(engine, lambda: _batch(engine, orders, 3))
    assert t[ONE]["count"] == 2, t
    _assert_same(got, _loop(engine, orders, 3), "1025 problems")


def test_same_order_overlap_and_leave_one_out(engine, oracle):
    X = _rows(oracle, 65, np.float64)
    _collect(engine, X)
    rng = np.random.default_rng(11)
    # every problem the same order: every problem equals problem 0 bit for bit
    one = _draw(rng, 300, 1, 100)
    same = np.repeat(one, 7, axis=0)
    got = _batch(engine, same, 30)
    _assert_same(got, _loop(engine, same[:1], 30) * 7, "same order")
    for b in range(1, 7):
        assert np.array_equal(got[0][b], got[0][0])
        assert _same_bits(got[1][b], got[1][0]) and _same_bits(got[2][b], got[2][0])
        assert _same_bits(got[3][b], got[3][0])
    # heavily overlapping subsets: 100 of the same 104 slots, each in its own order
    pool = rng.choice(300, size=104, replace=False)
    over = np.stack([rng.permutation(pool)[:100] for _ in range(7)]).astype(np.int64)
    _assert_same(_batch(engine, over, 30), _loop(engine, over, 30), "overlap")
    # leave-one-out of a 17-row collection
    _collect(engine, np.ascontiguousarray(X[:17]))
    loo = np.stack([np.delete(np.arange(17), b) for b in range(17)]).astype(np.int64)
    for f in (1, 5):
        _assert_same(_batch(engine, loo, f), _loop(engine, loo, f), ("leave one out", f))


def test_special_values_as_one_problem_of_four(engine, oracle):
    """the NaN-row and inf-row goldens of test_gpu_collect_small.py, each as one
    problem of a batch of four whose other problems are plain rows"""
    Xn, pn = GU.build_input("nan_row", oracle)
    Xi, pi = GU.build_input("inf_row", oracle)
    n, d, f = pn["n"], pn["d"], pn["f"]
    assert (pi["n"], pi["d"], pi["f"]) == (n, d, f)
    plain = oracle.synth(2 * n, d, 4242, 10)
    _collect(engine, np.ascontiguousarray(np.concatenate([Xn, plain, Xi])))
    rng = np.random.default_rng(3)
    base = {"nan_row": 0, "inf_row": 3 * n}
    for name, at in (("nan_row", 1), ("inf_row", 3), ("nan_row", 0), ("inf_row", 2)):
        orders = np.stack([n + rng.choice(2 * n, size=n, replace=False) for _ in range(4)])
        orders[at] = base[name] + np.arange(n)
        got = _batch(engine, orders.astype(np.int64), f)
        _assert_same(got, _loop(engine, orders, f), (name, at))
        assert np.array_equal(got[0][at], GU.load(name)["sel"]), (name, at)
    # both in one batch, and a problem that mixes the NaN row with plain rows
    orders = np.stack([np.arange(n), 3 * n + np.arange(n), n + np.arange(n),
                       np.concatenate([[5], n + np.arange(n - 1)])]).astype(np.int64)
    _assert_same(_batch(engine, orders, f), _loop(engine, orders, f), "nan and inf")


def test_nullable_outputs(engine, oracle):
    X = _rows(oracle, 65, np.float64)
    _collect(engine, X)
    orders = _draw(np.random.default_rng(5), 300, 3, 67)
    full = _loop(engine, orders, 20)
    for ws in (True, False):
        for wm in (True, False):
            got, t = _timed(engine, lambda: _batch(engine, orders, 20, ws, wm))
            assert t[ONE]["count"] == 1, t
            assert (got[1] is None) == (not ws) and (got[2] is None) == (not wm)
            _assert_same(got, full, (ws, wm))


def test_interleaving_and_repeat(engine, oracle):
    """its buffers are its own: a single finish, a bk_multikrum, a
    bk_multikrum_batch and a bk_collect_add between two batched finishes change
    nothing, and none of them is changed"""
    X = _rows(oracle, 7850, np.float64)
    n, f = 100, 30
    _collect(engine, np.ascontiguousarray(X[:200]), n_cap=300)
    orders = _draw(np.random.default_rng(17), 200, 3, n)
    ref = _loop(engine, orders, f)
    Y = np.ascontiguousarray(X[200:260])
    host_ref = engine.multikrum(Y, 20)
    Z = np.ascontiguousarray(X[260:300].reshape(2, 20, 7850))
    zb_ref = engine.multikrum_batch(Z, 6)
    zb_rec = _records(engine, 2)

    _assert_same(_batch(engine, orders, f), ref, "first")
    _assert_same(_batch(engine, orders, f), ref, "again, nothing between")
    one = engine.collect_finish(order=orders[1], f=f)
    assert np.array_equal(one[0], ref[1][0]) and _same_bits(one[2], ref[1][2])
    assert _same_bits(_record(engine), ref[1][3])
    _assert_same(_batch(engine, orders, f), ref, "after a single finish")
    got = engine.multikrum(Y, 20)
    assert np.array_equal(got[0], host_ref[0])
    assert _same_bits(got[1], host_ref[1]) and _same_bits(got[2], host_ref[2])
    _assert_same(_batch(engine, orders, f), ref, "after bk_multikrum")
    zb = engine.multikrum_batch(Z, 6)
    assert np.array_equal(zb[0], zb_ref[0])
    assert _same_bits(zb[1], zb_ref[1]) and _same_bits(zb[2], zb_ref[2])
    assert _same_bits(_records(engine, 2), zb_rec)
    _assert_same(_batch(engine, orders, f), ref, "after bk_multikrum_batch")
    assert engine.collect_add([X[200 + i] for i in range(100)]) == 200
    _assert_same(_batch(engine, orders, f), ref, "after bk_collect_add")
    wide = _draw(np.random.default_rng(18), 300, 3, n)
    assert wide.max() >= 200
    _assert_same(_batch(engine, wide, f), _loop(engine, wide, f), "the added rows")


def test_fallback_is_the_single_finish(engine, oracle):
    """n = 129, and bk_set_small_path(ctx, 0) at n = 100: the single finish per
    problem (the chain), bitwise, and no batched launch in the timing table"""
    X = _rows(oracle, 65, np.float64)
    _collect(engine, X)
    rng = np.random.default_rng(23)
    big = _draw(rng, 300, 3, 129)
    got, t = _timed(engine, lambda: _batch(engine, big, 40))
    assert ONE not in t and all(t[k]["count"] == 3 for k in CHAIN), t
    _assert_same(got, _loop(engine, big, 40), "n = 129")
    orders = _draw(rng, 300, 3, 100)
    ref = _loop(engine, orders, 30)  # the one-launch single finish
    engine.set_small_path(False)
    try:
        got, t = _timed(engine, lambda: _batch(engine, orders, 30))
        assert ONE not in t and all(t[k]["count"] == 3 for k in CHAIN), t
        chain = _loop(engine, orders, 30)
    finally:
        engine.set_small_path(True)
    _assert_same(got, chain, "small path off")
    _assert_same(got, ref, "small path off against the one-launch finish")
    _assert_same(_batch(engine, orders, 30), ref, "small path on again")


def test_errors_leave_everything_as_it_was(engine, oracle):
    X = _rows(oracle, 25, np.float64)
    _collect(engine, X)
    rng = np.random.default_rng(29)
    orders = _draw(rng, 300, 4, 16)
    ref = _loop(engine, orders, 5)
    _assert_same(_batch(engine, orders, 5), ref, "before")
    rec = _records(engine, 4)

    def unchanged(what):
        assert engine.collect_count() == 300
        assert _same_bits(_records(engine, 4), rec), what  # the last valid margin state
        _assert_same(_batch(engine, orders, 5), ref, what)

    bad = orders.copy()
    bad[2, 7] = 300  # no collected slot, in problem 2
    with pytest.raises(ValueError, match=r"problem 2.*order\[7\]"):
        engine.collect_finish_batch(bad, 5)
    unchanged("bad slot")
    bad[2, 7] = -1
    with pytest.raises(ValueError, match=r"problem 2.*order\[7\]"):
        engine.collect_finish_batch(bad, 5)
    unchanged("negative slot")
    rep = orders.copy()
    rep[3, 15] = rep[3, 4]  # a repeated slot in the last problem
    with pytest.raises(ValueError, match=r"problem 3.*order\[15\].*repeats"):
        engine.collect_finish_batch(rep, 5)
    unchanged("repeated slot")
    with pytest.raises(ValueError, match="rows collected"):  # n > count
        engine.collect_finish_batch(np.tile(np.arange(301), (2, 1)), 5)
    unchanged("n > count")
    sel = np.empty((4, 16), dtype=np.int64)
    st = _lib.lib().bk_collect_finish_batch(engine.ctx, orders.ctypes.data, 4, 16, 0,
                                            sel.ctypes.data, None, None, None)
    assert st == _lib.BK_EINVAL and "f=" in _lib.last_error(), _lib.last_error()
    unchanged("f = 0")
    st = _lib.lib().bk_collect_finish_batch(engine.ctx, None, 4, 16, 5, sel.ctypes.data, None,
                                            None, None)
    assert st == _lib.BK_EINVAL and "null orders" in _lib.last_error()
    st = _lib.lib().bk_collect_finish_batch(engine.ctx, orders.ctypes.data, 4, 16, 5, None, None,
                                            None, None)
    assert st == _lib.BK_EINVAL and "null sel_idx" in _lib.last_error()
    unchanged("null pointers")
    # a call without bk_collect_begin: a context of its own
    from biscotti_amd.krum import Engine
    fresh = Engine(engine.device)
    try:
        st = _lib.lib().bk_collect_finish_batch(fresh.ctx, orders.ctypes.data, 4, 16, 5,
                                                sel.ctypes.data, None, None, None)
        assert st == _lib.BK_EINVAL and "without bk_collect_begin" in _lib.last_error()
    finally:
        fresh.close()
    unchanged("without begin")


def _picked(recs):
    """bk_multikrum_batch's rule: the lowest-index near tie, else the smallest
    gap - err_bound (no record here carries an error code)"""
    tie = np.flatnonzero(recs[:, 2] != 0.0)
    if tie.size:
        return int(tie[0])
    return int(np.argmin(recs[:, 0] - recs[:, 1]))


def test_margins(engine, oracle):
    """bk_selection_margin_batch equals the single finishes' records row for row
    (every case above asserts that too); bk_selection_margin / _record report
    the lowest-index near tie, else the smallest gap - err_bound"""
    X = np.array(_rows(oracle, 64, np.float64)[:40])
    # three pairs of equal rows: in a problem of exactly these six the scores
    # come in three equal pairs, so with f = 1 (m = 5) the boundary falls inside
    # the last pair -- a gap of exactly 0; with k = 3 no other problem ties
    X[30], X[31], X[32] = X[3], X[9], X[14]
    _collect(engine, X)
    rng = np.random.default_rng(31)
    # no near tie anywhere: the smallest gap - err_bound
    orders = _draw(rng, 30, 5, 6)
    ref = _loop(engine, orders, 1)
    assert not any(r[3][2] for r in ref)
    got = _batch(engine, orders, 1)
    _assert_same(got, ref, "no tie")
    pick = _picked(got[3])
    assert pick == int(np.argmin([r[3][0] - r[3][1] for r in ref]))
    assert _same_bits(_record(engine), got[3][pick])
    m = engine.selection_margin()
    assert not m["near_tie"] and m["gap"] == got[3][pick][0]
    # exactly one near tie, at problem 2, and not the smallest gap - err_bound's problem
    orders[2] = [3, 30, 9, 31, 14, 32]
    ref = _loop(engine, orders, 1)
    assert [bool(r[3][2]) for r in ref] == [False, False, True, False, False]
    got = _batch(engine, orders, 1)
    _assert_same(got, ref, "one tie")
    assert _same_bits(_record(engine), got[3][2])
    m = engine.selection_margin()
    assert m["near_tie"] and m["gap"] == 0.0
    # two near ties: the lower index
    orders[4] = [32, 31, 9, 30, 14, 3]
    ref = _loop(engine, orders, 1)
    got = _batch(engine, orders, 1)  # (the batch last: the margin calls below report it)
    _assert_same(got, ref, "two ties")
    assert got[3][4][2] != 0.0 and _same_bits(_record(engine), got[3][2])
    # the k = 0 problem (n = 3, f = 1): every score is 0, so every problem is a
    # near tie and problem 0's record is the one reported
    k0 = _draw(rng, 40, 3, 3)
    ref = _loop(engine, k0, 1)
    got = _batch(engine, k0, 1)
    _assert_same(got, ref, "k = 0")
    assert all(got[3][:, 2] != 0.0) and all(got[3][:, 7] == 0.0)
    assert _same_bits(_record(engine), got[3][0])
    assert engine.selection_margin()["near_tie"]
    # the fallback loop keeps the same rule
    engine.set_small_path(False)
    try:
        got = _batch(engine, orders, 1)
        assert _same_bits(_record(engine), got[3][2])
    finally:
        engine.set_small_path(True)
    with pytest.raises(ValueError):  # another problem count than the last call's
        _records(engine, 4)


def test_anchor_against_packed_multikrum(engine, oracle):
    """independent of the single finish: each problem's sel and mean are bitwise
    bk_multikrum's on the rows packed in that problem's order (the collection's
    contract, wherever the problem reports no near tie)"""
    X = _rows(oracle, 7850, np.float64)
    _collect(engine, X)
    orders = _draw(np.random.default_rng(37), 300, 3, 100)
    sel, sc, mean, recs = _batch(engine, orders, 30)
    checked = 0
    for b in range(3):
        if recs[b][2] != 0.0:
            continue
        ps, _, pm = engine.multikrum(np.ascontiguousarray(X[orders[b]]), 30)
        assert np.array_equal(sel[b], ps), b
        assert _same_bits(mean[b], pm), b
        checked += 1
    assert checked == 3  # synthetic rows with a 60-row Byzantine cluster: no near tie
