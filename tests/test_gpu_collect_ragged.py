"""bk_collect_finish_ragged (k_collect_small_ragged, bk_collect_ragged.hip): many
finishes over ONE collection in one call, each problem with its own n and f --
k_collect_small's S and M items behind a per-problem descriptor, one launch
sequence per bucket NB = ceil(n / 16), every output at the caller's position.

The bar, in every case: each problem's sel, scores, mean and all eight margin
fields are BITWISE what bk_collect_finish gives on that problem alone on the same
context and collection.  Every comparison is exact equality of bits (doubles
through view(uint64), so NaNs compare too); no tolerance appears anywhere."""
import ctypes

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

ONE = "k_small"  # BK_K_SMALL as bk_timing_read names it: the ragged launches are timed under it
CHAIN = ("k_scores", "k_rank", "k_compact")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _record(engine):
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _records(engine, batch):
    rec = (ctypes.c_double * (8 * batch))()
    _lib.check(_lib.lib().bk_selection_margin_batch(engine.ctx, rec, batch))
    return np.array(list(rec), dtype=np.float64).reshape(batch, 8)


# the collection now on the session's engine, so that consecutive cases on the
# same rows add them once (any other module's test begins its own)
_ON = {"key": None}


@pytest.fixture(autouse=True, scope="module")
def _forget_collection():
    _ON["key"] = None
    yield
    _ON["key"] = None


def _collect(engine, X, key=None, n_cap=None):
    if key is not None and _ON["key"] == key:
        return
    n, d = X.shape
    engine.collect_begin(n_cap or n, d, X.dtype)
    for i in range(0, n, 30):
        assert engine.collect_add([X[r] for r in range(i, min(n, i + 30))]) == i
    assert engine.collect_count() == n
    _ON["key"] = key


# one 300-row collection per (d, dtype), its rows built once per module
_ROWS = {}


def _rows(oracle, d, dtype):
    key = (d, np.dtype(dtype).name)
    if key not in _ROWS:
        X = oracle.synth(300, d, 9000 + d, 60, dtype=dtype)
        X.setflags(write=False)
        _ROWS[key] = X
    return _ROWS[key]


def _shared(engine, oracle, d, dtype=np.float64):
    X = _rows(oracle, d, dtype)
    _collect(engine, X, key=(d, np.dtype(dtype).name))
    return X


def _fs(orders, fs):
    return [int(fs)] * len(orders) if np.ndim(fs) == 0 else [int(f) for f in fs]


def _loop(engine, orders, fs, ws=True, wm=True):
    """the reference: one bk_collect_finish per problem"""
    out = []
    for o, f in zip(orders, _fs(orders, fs)):
        sel, sc, mean = engine.collect_finish(order=np.ascontiguousarray(o, dtype=np.int64), f=f,
                                              want_scores=ws, want_mean=wm)
        out.append((sel, sc, mean, _record(engine)))
    return out


def _ragged(engine, orders, fs, ws=True, wm=True):
    sels, scs, mean = engine.collect_finish_ragged(orders, fs, want_scores=ws, want_mean=wm)
    return sels, scs, mean, _records(engine, len(orders))


def _raw(engine, orders, fs, ws=True, wm=True, wmo=True, d=None):
    """the C entry itself: packed arrays in, packed arrays out"""
    fs = np.array(_fs(orders, fs), dtype=np.int64)
    ns = np.array([len(o) for o in orders], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    packed = np.ascontiguousarray(np.concatenate(orders), dtype=np.int64)
    B = len(orders)
    sel = np.full(int((ns - fs).sum()), -99, dtype=np.int64)
    mo = np.full(B, -99, dtype=np.int64) if wmo else None
    sc = np.full(int(off[B]), 7.0) if ws else None
    mean = np.full((B, d), 7.0) if wm else None
    _lib.check(_lib.lib().bk_collect_finish_ragged(
        engine.ctx, packed.ctypes.data, off.ctypes.data, fs.ctypes.data, B, sel.ctypes.data,
        mo.ctypes.data if wmo else None, sc.ctypes.data if ws else None,
        mean.ctypes.data if wm else None))
    return sel, mo, sc, mean, _records(engine, B)


def _assert_same(got, ref, what):
    sels, scs, mean, recs = got
    assert len(sels) == len(ref) == recs.shape[0], what
    for b, (rs, rsc, rm, rrec) in enumerate(ref):
        assert sels[b].dtype == np.int64 and np.array_equal(sels[b], rs), (what, b, "sel", sels[b], rs)
        if scs is not None and rsc is not None:
            assert _same_bits(scs[b], rsc), (what, b, "scores")
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


def _draw(rng, count, ns):
    """a random subset in random order per problem: slots >= 128 occur once count > 128"""
    return [rng.choice(count, size=int(n), replace=False).astype(np.int64) for n in ns]


def _buckets(orders):
    """launch sequences a call takes: the NB buckets with two or more problems
    (all within the one-launch range), and the problems that run the single finish"""
    nb = {}
    for o in orders:
        if len(o) <= 128:
            nb[(len(o) + 15) // 16] = nb.get((len(o) + 15) // 16, 0) + 1
    shared = sum(1 for v in nb.values() if v >= 2)
    small_single = sum(1 for v in nb.values() if v == 1)
    return shared, small_single


MIXED_N = (2, 3, 16, 17, 32, 33, 100, 112, 113, 128)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 25, 64, 65, 7850])
def test_bitwise_against_the_single_finish(engine, oracle, d, dtype):
    """Fails without the feature.  ONE call mixing every n_b at an NB edge and
    both ends of the range with f_b = 1, n_b - 1 (m = 1) and n_b / 2 (n = 3,
    f = 1 and n = 2: k = 0, every score 0, the tie rule decides); d over one M
    item, the 64-column boundaries and more items than CUs; random subsets of
    a 300-row collection, so slots >= 128 occur"""
    _shared(engine, oracle, d, dtype)
    rng = np.random.default_rng(2000 + d)
    ns, fs = [], []
    for n in MIXED_N:
        for f in sorted({1, n - 1, n // 2}):
            ns.append(n)
            fs.append(f)
    orders = _draw(rng, 300, ns)
    assert max(int(o.max()) for o in orders) >= 128
    got, t = _timed(engine, lambda: _ragged(engine, orders, fs))
    # buckets 1 (n = 2, 3, 16), 2 (17, 32), 3 (33), 7 (100, 112), 8 (113, 128)
    assert _buckets(orders) == (5, 0)
    assert t[ONE]["count"] == 5 and not any(k in t for k in CHAIN), t
    assert [len(s) for s in got[0]] == [n - f for n, f in zip(ns, fs)]
    assert [len(s) for s in got[1]] == ns and got[2].shape == (len(ns), d)
    _assert_same(got, _loop(engine, orders, fs), (d, np.dtype(dtype).name))
    k0 = [b for b, (n, f) in enumerate(zip(ns, fs)) if n - f - 2 <= 0]
    assert k0 and all(not got[1][b].any() for b in k0)


def test_use_cases(engine, oracle):
    _shared(engine, oracle, 25)
    rng = np.random.default_rng(41)
    arrival = rng.permutation(300).astype(np.int64)
    # the deadline's verdict after each arrival
    prefixes = [arrival[:j] for j in range(2, 41)]
    fs = [j // 2 for j in range(2, 41)]
    got, t = _timed(engine, lambda: _ragged(engine, prefixes, fs))
    assert t[ONE]["count"] == 3, t  # n = 2..16, 17..32, 33..40
    _assert_same(got, _loop(engine, prefixes, fs), "prefixes")
    # an f sweep over one fixed order: one bucket, n the same, f free
    for n in (17, 100):
        order = arrival[:n]
        sweep = list(range(1, n))
        got, t = _timed(engine, lambda: _ragged(engine, [order] * (n - 1), sweep))
        assert t[ONE]["count"] == 1, t
        _assert_same(got, _loop(engine, [order] * (n - 1), sweep), ("f sweep", n))
    # the full set next to a 70-slot deadline subset
    both = [np.arange(300, dtype=np.int64), arrival[:70]]
    _assert_same(_ragged(engine, both, [150, 35]), _loop(engine, both, [150, 35]), "full + subset")


def test_bucket_mechanics(engine, oracle):
    _shared(engine, oracle, 25)
    rng = np.random.default_rng(43)
    # one bucket, 16 different n_b, f free
    ns = list(range(97, 113))
    fs = [int(rng.integers(1, n)) for n in ns]
    orders = _draw(rng, 300, ns)
    got, t = _timed(engine, lambda: _ragged(engine, orders, fs))
    assert t[ONE]["count"] == 1, t
    _assert_same(got, _loop(engine, orders, fs), "16 sizes, one bucket")
    # a bucket with exactly one problem: the single finish for it, one ragged
    # launch for the other two, both timed under k_small
    orders = _draw(rng, 300, [10, 40, 12])
    assert _buckets(orders) == (1, 1)
    got, t = _timed(engine, lambda: _ragged(engine, orders, [3, 11, 5]))
    assert t[ONE]["count"] == 2 and not any(k in t for k in CHAIN), t
    _assert_same(got, _loop(engine, orders, [3, 11, 5]), "a bucket of one")
    # descending and shuffled n_b over four buckets: every output at the caller's position
    ns = [128, 113, 100, 97, 40, 33, 17, 16, 9, 2]
    for order_of in (np.arange(len(ns)), rng.permutation(len(ns))):
        nn = [ns[i] for i in order_of]
        fs = [max(1, n // 3) for n in nn]
        orders = _draw(rng, 300, nn)
        _assert_same(_ragged(engine, orders, fs), _loop(engine, orders, fs), ("order", nn))


def test_two_launches_past_1024_problems(engine, oracle):
    """1,025 problems of one bucket, n_b in 9..16 at d = 25: launches of at most
    1,024 problems, so two of them, shown by the timing table"""
    _shared(engine, oracle, 25)
    rng = np.random.default_rng(47)
    ns = rng.integers(9, 17, size=1025)
    fs = [int(rng.integers(1, n)) for n in ns]
    orders = _draw(rng, 300, ns)
    got, t = _timed(engine, lambda: _ragged(engine, orders, fs))
    assert t[ONE]["count"] == 2, t
    _assert_same(got, _loop(engine, orders, fs), "1025 problems")


def test_routing(engine, oracle):
    _shared(engine, oracle, 65)
    rng = np.random.default_rng(53)
    # n = 129 and n = 200 (the chain) among small ones
    ns, fs = [20, 129, 100, 200, 30, 101], [6, 40, 30, 90, 14, 50]
    orders = _draw(rng, 300, ns)
    ref = _loop(engine, orders, fs)
    got, t = _timed(engine, lambda: _ragged(engine, orders, fs))
    assert t[ONE]["count"] == 2 and all(t[k]["count"] == 2 for k in CHAIN), t
    _assert_same(got, ref, "129 and 200 among small ones")
    # the small path off: no ragged launch, the chain per problem, the same bits
    engine.set_small_path(False)
    try:
        got, t = _timed(engine, lambda: _ragged(engine, orders, fs))
        assert ONE not in t and all(t[k]["count"] == 6 for k in CHAIN), t
    finally:
        engine.set_small_path(True)
    _assert_same(got, ref, "small path off")
    _assert_same(_ragged(engine, orders, fs), ref, "small path on again")
    # batch = 1: the single finish
    got, t = _timed(engine, lambda: _ragged(engine, orders[2:3], fs[2:3]))
    assert t[ONE]["count"] == 1, t
    _assert_same(got, ref[2:3], "batch = 1")
    assert _same_bits(_record(engine), ref[2][3])


def test_uniform_input_equals_the_uniform_entry(engine, oracle):
    _shared(engine, oracle, 65)
    rng = np.random.default_rng(59)
    for n, f, B in ((100, 30, 7), (16, 5, 3), (3, 1, 4)):
        orders = np.stack(_draw(rng, 300, [n] * B))
        sel, sc, mean = engine.collect_finish_batch(orders, f)
        recs = _records(engine, B)
        got = _ragged(engine, list(orders), f)
        for b in range(B):
            assert np.array_equal(got[0][b], sel[b]) and _same_bits(got[1][b], sc[b]), (n, b)
            assert _same_bits(got[2][b], mean[b]) and _same_bits(got[3][b], recs[b]), (n, b)


def test_special_values_as_one_problem_of_four(engine, oracle):
    """the NaN-row and inf-row goldens of test_gpu_collect_small.py, each as one
    problem of four whose other problems are plain rows of other sizes"""
    Xn, pn = GU.build_input("nan_row", oracle)
    Xi, pi = GU.build_input("inf_row", oracle)
    n, d, f = pn["n"], pn["d"], pn["f"]
    assert (pi["n"], pi["d"], pi["f"]) == (n, d, f)
    plain = oracle.synth(2 * n, d, 4242, 10)
    _collect(engine, np.ascontiguousarray(np.concatenate([Xn, plain, Xi])))
    rng = np.random.default_rng(3)
    base = {"nan_row": 0, "inf_row": 3 * n}
    others = [max(3, n - 1), min(2 * n, n + 1), max(3, n // 2)]
    for name, at in (("nan_row", 1), ("inf_row", 3), ("nan_row", 0), ("inf_row", 2)):
        ns = others[:at] + [n] + others[at:]
        orders = [n + rng.choice(2 * n, size=q, replace=False) for q in ns]
        orders[at] = base[name] + np.arange(n)
        fs = [f if q == n else max(1, q // 3) for q in ns]
        got = _ragged(engine, orders, fs)
        _assert_same(got, _loop(engine, orders, fs), (name, at))
        assert np.array_equal(got[0][at], GU.load(name)["sel"]), (name, at)
    # both in one call, and a problem that mixes the NaN row with plain rows
    orders = [np.arange(n), 3 * n + np.arange(n), n + np.arange(n + 1),
              np.concatenate([[5], n + np.arange(n - 2)])]
    fs = [f, f, max(1, n // 3), max(1, n // 3)]
    _assert_same(_ragged(engine, orders, fs), _loop(engine, orders, fs), "nan and inf")


def test_nullable_outputs(engine, oracle):
    _shared(engine, oracle, 65)
    rng = np.random.default_rng(61)
    ns, fs = [67, 70, 20, 129], [20, 35, 1, 60]
    orders = _draw(rng, 300, ns)
    ref = _loop(engine, orders, fs)
    off = np.concatenate([[0], np.cumsum(ns)])
    so = np.concatenate([[0], np.cumsum(np.array(ns) - np.array(fs))])
    for ws, wm, wmo in ((True, False, False), (False, True, False), (False, False, True),
                        (False, False, False), (True, True, True)):
        sel, mo, sc, mean, recs = _raw(engine, orders, fs, ws, wm, wmo, d=65)
        for b, (rs, rsc, rm, rrec) in enumerate(ref):
            assert np.array_equal(sel[so[b]:so[b + 1]], rs), (ws, wm, wmo, b)
            assert _same_bits(recs[b], rrec)
            if ws:
                assert _same_bits(sc[off[b]:off[b + 1]], rsc), (ws, wm, wmo, b)
            if wm:
                assert _same_bits(mean[b], rm), (ws, wm, wmo, b)
        if wmo:
            assert np.array_equal(mo, np.array(ns) - np.array(fs))


def test_isolation(engine, oracle):
    """its buffers are the collection's own: a single finish, a batched finish, a
    bk_multikrum, a bk_multikrum_batch and a bk_collect_add between two ragged
    calls change nothing, and none of them is changed"""
    X = _rows(oracle, 7850, np.float64)
    _collect(engine, np.ascontiguousarray(X[:200]), n_cap=300)
    rng = np.random.default_rng(67)
    ns, fs = [100, 97, 20, 17, 30], [30, 40, 6, 8, 1]
    orders = _draw(rng, 200, ns)
    ref = _loop(engine, orders, fs)
    uni = np.stack(_draw(rng, 200, [50] * 3))
    ub_ref = engine.collect_finish_batch(uni, 20)
    ub_rec = _records(engine, 3)
    Y = np.ascontiguousarray(X[200:260])
    host_ref = engine.multikrum(Y, 20)
    Z = np.ascontiguousarray(X[260:300].reshape(2, 20, 7850))
    zb_ref = engine.multikrum_batch(Z, 6)
    zb_rec = _records(engine, 2)

    _assert_same(_ragged(engine, orders, fs), ref, "first")
    _assert_same(_ragged(engine, orders, fs), ref, "again, nothing between")
    one = engine.collect_finish(order=orders[1], f=fs[1])
    assert np.array_equal(one[0], ref[1][0]) and _same_bits(one[2], ref[1][2])
    assert _same_bits(_record(engine), ref[1][3])
    _assert_same(_ragged(engine, orders, fs), ref, "after a single finish")
    ub = engine.collect_finish_batch(uni, 20)
    assert all(_same_bits(a, b) for a, b in zip(ub[1:], ub_ref[1:])) and np.array_equal(ub[0], ub_ref[0])
    assert _same_bits(_records(engine, 3), ub_rec)
    _assert_same(_ragged(engine, orders, fs), ref, "after bk_collect_finish_batch")
    got = engine.multikrum(Y, 20)
    assert np.array_equal(got[0], host_ref[0])
    assert _same_bits(got[1], host_ref[1]) and _same_bits(got[2], host_ref[2])
    _assert_same(_ragged(engine, orders, fs), ref, "after bk_multikrum")
    zb = engine.multikrum_batch(Z, 6)
    assert np.array_equal(zb[0], zb_ref[0])
    assert _same_bits(zb[1], zb_ref[1]) and _same_bits(zb[2], zb_ref[2])
    assert _same_bits(_records(engine, 2), zb_rec)
    _assert_same(_ragged(engine, orders, fs), ref, "after bk_multikrum_batch")
    assert engine.collect_add([X[200 + i] for i in range(3)]) == 200
    _assert_same(_ragged(engine, orders, fs), ref, "after bk_collect_add")
    wide = _draw(rng, 203, ns)
    wide[0][0], wide[3][5] = 202, 201
    wide = [np.array(list(dict.fromkeys(o.tolist())), dtype=np.int64) for o in wide]
    wfs = [min(f, len(o) - 1) for f, o in zip(fs, wide)]
    _assert_same(_ragged(engine, wide, wfs), _loop(engine, wide, wfs), "the added rows")


def test_errors_leave_everything_as_it_was(engine, oracle):
    _shared(engine, oracle, 25)
    rng = np.random.default_rng(71)
    ns, fs = [16, 12, 20, 9], [5, 3, 8, 2]
    orders = _draw(rng, 300, ns)
    ref = _loop(engine, orders, fs)
    _assert_same(_ragged(engine, orders, fs), ref, "before")
    rec, picked = _records(engine, 4), _record(engine)

    def unchanged(what):
        assert engine.collect_count() == 300
        assert _same_bits(_records(engine, 4), rec), what  # the last valid margin state
        assert _same_bits(_record(engine), picked), what
        _assert_same(_ragged(engine, orders, fs), ref, what)

    L = _lib.lib()
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    packed = np.concatenate(orders).astype(np.int64)
    fa = np.array(fs, dtype=np.int64)
    sel = np.empty(64, dtype=np.int64)

    def call(ctx=engine.ctx, o=packed, of=off, f=fa, batch=4, s=sel):
        return L.bk_collect_finish_ragged(ctx, o.ctypes.data if o is not None else None,
                                          of.ctypes.data if of is not None else None,
                                          f.ctypes.data if f is not None else None, batch,
                                          s.ctypes.data if s is not None else None, None, None,
                                          None)

    # 1. the batch, before the pointers
    assert call(o=None, of=None, f=None, batch=0, s=None) == _lib.BK_EINVAL
    assert "batch" in _lib.last_error()
    assert call(o=None, batch=_lib.BK_MAX_BATCH + 1) == _lib.BK_ENOTSUP
    unchanged("batch")
    # 2. the pointers, by name
    for kw, word in (({"o": None}, "null orders"), ({"of": None}, "null offsets"),
                     ({"f": None}, "null fs"), ({"s": None}, "null sel_idx")):
        assert call(**kw) == _lib.BK_EINVAL and word in _lib.last_error(), _lib.last_error()
    unchanged("null pointers")
    # 3. a call without bk_collect_begin: a context of its own
    from biscotti_amd.krum import Engine
    fresh = Engine(engine.device)
    try:
        assert call(ctx=fresh.ctx) == _lib.BK_EINVAL
        assert "without bk_collect_begin" in _lib.last_error()
    finally:
        fresh.close()
    unchanged("without begin")
    # 4. the offsets
    bad = off.copy()
    bad[0] = 1
    assert call(of=bad) == _lib.BK_EINVAL and "offsets[0]" in _lib.last_error()
    bad = off.copy()
    bad[2] = bad[1]  # problem 1 empty
    assert call(of=bad) == _lib.BK_EINVAL and "problem 1" in _lib.last_error(), _lib.last_error()
    bad = off.copy()
    bad[3] = bad[2] - 1  # problem 2 negative
    assert call(of=bad) == _lib.BK_EINVAL and "problem 2" in _lib.last_error()
    big = [np.arange(5), np.arange(301) % 300]
    with pytest.raises(ValueError, match=r"problem 1.*rows collected"):  # n_b > count
        engine.collect_finish_ragged(big, 2)
    unchanged("offsets")
    # 5. bk_check_args, per problem
    for f_bad in (0, 20, -1):
        bf = fa.copy()
        bf[2] = f_bad
        assert call(f=bf) == _lib.BK_EINVAL
        assert _lib.last_error().startswith("problem 2: ") and "f=" in _lib.last_error()
    unchanged("f outside bk_check_args")
    # 6. the slots
    bo = [o.copy() for o in orders]
    bo[2][7] = 300
    with pytest.raises(ValueError, match=r"problem 2.*order\[7\]"):
        engine.collect_finish_ragged(bo, fs)
    bo[2][7] = -1
    with pytest.raises(ValueError, match=r"problem 2.*order\[7\]"):
        engine.collect_finish_ragged(bo, fs)
    bo = [o.copy() for o in orders]
    bo[3][8] = bo[3][4]
    with pytest.raises(ValueError, match=r"problem 3.*order\[8\].*repeats"):
        engine.collect_finish_ragged(bo, fs)
    unchanged("slots")
    # a slot used by two problems is no error
    bo = [o.copy() for o in orders]
    bo[1] = bo[0][:12].copy()
    _assert_same(_ragged(engine, bo, fs), _loop(engine, bo, fs), "shared slots")


def _picked(recs):
    """bk_multikrum_batch's rule: the lowest-index near tie, else the smallest
    gap - err_bound (no record here carries an error code)"""
    tie = np.flatnonzero(recs[:, 2] != 0.0)
    if tie.size:
        return int(tie[0])
    return int(np.argmin(recs[:, 0] - recs[:, 1]))


def test_margins(engine, oracle):
    """bk_selection_margin_batch gives the single finishes' records in the
    caller's order (every case above asserts that too); bk_selection_margin /
    _record report the lowest-index near tie, else the smallest gap - err_bound"""
    X = np.array(_rows(oracle, 64, np.float64)[:40])
    # three pairs of equal rows: in a problem of exactly these six the scores
    # come in three equal pairs, so with f = 1 (m = 5) the boundary falls inside
    # the last pair -- a gap of exactly 0
    X[30], X[31], X[32] = X[3], X[9], X[14]
    _collect(engine, X)
    rng = np.random.default_rng(73)
    ns = [7, 20, 6, 17, 9]
    fs = [1, 6, 1, 5, 2]
    orders = _draw(rng, 30, ns)
    ref = _loop(engine, orders, fs)
    assert not any(r[3][2] for r in ref)  # no near tie anywhere
    got = _ragged(engine, orders, fs)
    _assert_same(got, ref, "no tie")
    pick = _picked(got[3])
    assert pick == int(np.argmin([r[3][0] - r[3][1] for r in ref]))
    assert _same_bits(_record(engine), got[3][pick])
    m = engine.selection_margin()
    assert not m["near_tie"] and m["gap"] == got[3][pick][0]
    # exactly one near tie, at problem 2
    orders[2] = np.array([3, 30, 9, 31, 14, 32], dtype=np.int64)
    ref = _loop(engine, orders, fs)
    assert [bool(r[3][2]) for r in ref] == [False, False, True, False, False]
    got = _ragged(engine, orders, fs)
    _assert_same(got, ref, "one tie")
    assert _same_bits(_record(engine), got[3][2])
    m = engine.selection_margin()
    assert m["near_tie"] and m["gap"] == 0.0
    # two near ties: the lower index in the caller's order
    orders[4] = np.array([32, 31, 9, 30, 14, 3], dtype=np.int64)
    fs[4] = 1
    ref = _loop(engine, orders, fs)
    got = _ragged(engine, orders, fs)
    _assert_same(got, ref, "two ties")
    assert got[3][4][2] != 0.0 and _same_bits(_record(engine), got[3][2])
    # a k = 0 problem (n = 3, f = 1: every score 0, a near tie) ahead of them in
    # the caller's order, behind a problem of another bucket
    orders2 = [orders[1], rng.choice(30, size=3, replace=False).astype(np.int64)] + orders[2:]
    fs2 = [fs[1], 1] + fs[2:]
    ref = _loop(engine, orders2, fs2)
    got = _ragged(engine, orders2, fs2)
    _assert_same(got, ref, "k = 0")
    assert got[3][1][2] != 0.0 and got[3][1][7] == 0.0
    assert _same_bits(_record(engine), got[3][1])
    assert engine.selection_margin()["near_tie"]
    with pytest.raises(ValueError):  # another problem count than the last call's
        _records(engine, 4)


def test_engine_returns_against_the_c_entry(engine, oracle):
    _shared(engine, oracle, 65)
    rng = np.random.default_rng(79)
    ns, fs = [33, 5, 128, 40], [10, 2, 64, 13]
    orders = _draw(rng, 300, ns)
    sel, mo, sc, mean, recs = _raw(engine, orders, fs, d=65)
    off = np.concatenate([[0], np.cumsum(ns)])
    so = np.concatenate([[0], np.cumsum(mo)])
    sels, scs, mean2 = engine.collect_finish_ragged(orders, fs)
    assert isinstance(sels, list) and isinstance(scs, list) and mean2.shape == (4, 65)
    for b in range(4):
        assert sels[b].dtype == np.int64 and np.array_equal(sels[b], sel[so[b]:so[b + 1]])
        assert scs[b].dtype == np.float64 and _same_bits(scs[b], sc[off[b]:off[b + 1]])
    assert _same_bits(mean2, mean) and _same_bits(_records(engine, 4), recs)
    # fs as one int; nothing wanted
    sels, scs, mean2 = engine.collect_finish_ragged(orders, 2, want_scores=False, want_mean=False)
    assert scs is None and mean2 is None
    _assert_same((sels, None, None, _records(engine, 4)), _loop(engine, orders, 2), "fs = 2")
