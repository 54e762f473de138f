"""The last arrival as Delta and Noise, noised and finished in one call
(bk_collect_add_noised_finish, bk_collect_arrive_noised.hip): the copies, then
ONE launch -- k_collect_arrive_noised, the noise of the new row and its border
in front of k_collect_small's work items.

The bar: collect_stats() and the timing table show the path taken; every output
-- sel, scores, mean and the eight margin fields -- is BITWISE what
bk_collect_add_noised followed by bk_collect_finish gives on the same engine
after a fresh bk_collect_begin with the same rows (the reference of every check
here, never the fused call itself and never a second evaluation of the noise),
and so is the stored row and everything a later add or finish sees."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import Engine, KRUMValidator, Update  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"
FUSED = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 1}
TWO_SMALL = {"border": 1, "border_reduce": 1, "one_launch_finishes": 1, "fused_arrivals": 0}
TWO_CHAIN = {"border": 1, "border_reduce": 1, "one_launch_finishes": 0, "fused_arrivals": 0}
WHERES = (_lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE)
BK_K_NOISE = 13


def _path(where, d, k):
    """the path a call in k_collect_small's range takes: host rows of more than
    32 KiB were measured ahead on the fused launch only pinned with k = 1 and
    take the two calls inside the entry otherwise"""
    if where == _lib.BK_DEVICE or d * 8 <= 32768 or (where == _lib.BK_HOST_PINNED and k == 1):
        return FUSED
    return TWO_SMALL


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


def _same_bits(a, b):
    """bitwise but for the payload of a NaN: a NaN matches a NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _assert_bitwise(got, ref, what):
    (gs, gsc, gm), grec = got
    (rs, rsc, rm), rrec = ref
    assert np.array_equal(gs, rs), (what, "sel", gs, rs)
    if gm is not None and rm is not None:
        assert _same_bits(gm, rm), (what, "mean")
    assert _same_record(grec, rrec), (what, "margin", grec, rrec)
    if gsc is not None and rsc is not None:
        assert _same_bits(gsc, rsc), (what, "scores", gsc, rsc)


def _begin(engine, X, upto, n_cap=None, group=30):
    """a fresh collection holding rows 0..upto-1 of X (resident rows: plain adds)"""
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


class _Arrival:
    """one update's delta and k noise vectors in `where` memory and their
    pointers.  Pageable and device noise vectors start one double past a 16-byte
    boundary (8-B but not 16-B aligned), the delta on one"""

    def __init__(self, delta, noise, where):
        self.where = where
        self.k = noise.shape[0]
        self.keep = []
        self.dptr = self._row(delta, 0)
        self.nptr = [self._row(noise[j], 1) for j in range(self.k)]
        if where == _lib.BK_DEVICE:
            torch.cuda.synchronize()
            assert all(p % 16 == 8 for p in self.nptr)

    def _row(self, v, odd):
        d = v.shape[0]
        if self.where == _lib.BK_HOST:
            buf = np.empty(d + 3, dtype=np.float64)
            odd += (buf.ctypes.data % 16) // 8  # numpy gives 16-B alignment or not
            a = buf[odd:odd + d]
            a[:] = v
            self.keep.append(buf)
            return a.ctypes.data
        t = torch.empty(d + 1, dtype=torch.float64)
        t[odd:odd + d] = torch.from_numpy(np.array(v))
        t = t.pin_memory() if self.where == _lib.BK_HOST_PINNED else t.cuda()
        self.keep.append(t)
        return t.data_ptr() + 8 * odd

    def _nz(self):
        return (ctypes.c_void_p * self.k)(*self.nptr) if self.k else None

    def add(self, engine):
        dp = (ctypes.c_void_p * 1)(self.dptr)
        return engine.collect_add_noised_ptr(dp, self._nz(), self.k, 1, self.where)

    def add_finish(self, engine, d, order=None, n=None, f=None, want_scores=True, want_mean=True):
        """collect_add_noised_finish_ptr -> (slot, sel, scores, mean)"""
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.int64)
            n = len(order) if n is None else n
        elif n is None:
            n = engine.collect_count() + 1
        sel = np.empty(n - f, np.int64)
        sc = np.empty(n) if want_scores else None
        mean = np.empty(d) if want_mean else None
        slot, m = engine.collect_add_noised_finish_ptr(
            self.dptr, self._nz(), self.k, self.where,
            order.ctypes.data if order is not None else None, n, f, sel.ctypes.data,
            sc.ctypes.data if sc is not None else None,
            mean.ctypes.data if mean is not None else None)
        assert m == n - f
        return slot, sel, sc, mean


def _two_calls(engine, X, j, arr, n_cap=None, **kw):
    """THE REFERENCE: rows 0..j-1 collected afresh, then the noised add of the
    arrival and collect_finish(**kw) -> ((sel, scores, mean), record), the
    launches taken, the stored row"""
    _begin(engine, X, j, n_cap)
    s0 = engine.collect_stats()
    assert arr.add(engine) == j
    out = _finish(engine, **kw)
    return out, _delta(engine.collect_stats(), s0), engine.collect_read_rows([j])[0]


def _fused(engine, X, j, arr, n_cap=None, **kw):
    """rows 0..j-1 collected afresh, then the one call"""
    _begin(engine, X, j, n_cap)
    s0 = engine.collect_stats()
    slot, sel, sc, mean = arr.add_finish(engine, X.shape[1], **kw)
    assert slot == j and engine.collect_count() == j + 1
    return (((sel, sc, mean), _record(engine)), _delta(engine.collect_stats(), s0),
            engine.collect_read_rows([j])[0])


def _both(engine, X, j, arr, what, path=FUSED, n_cap=None, **kw):
    """the one call against the reference, bitwise, on the expected path"""
    ref, rs, rrow = _two_calls(engine, X, j, arr, n_cap, **kw)
    got, gs, grow = _fused(engine, X, j, arr, n_cap, **kw)
    assert gs == path, (what, gs)
    _assert_bitwise(got, ref, what)
    assert _same_bits(grow, rrow), (what, "stored row")
    return got, ref, rs, grow


_cases = {}


def _case(oracle, n, d, k, seed=0):
    """(resident rows X, the arrival's delta, its (k, d) noise), computed once
    per shape and never modified"""
    key = (n, d, k, seed)
    if key not in _cases:
        X = oracle.synth(n, d, 900 + n + d + k + seed, max(1, n // 4))
        rng = np.random.default_rng(7 * d + 3 * k + n + seed)
        delta = np.ascontiguousarray(X[n - 1])
        noise = 1e-2 * rng.standard_normal((k, d))
        for a in (X, delta, noise):
            a.setflags(write=False)
        _cases[key] = (X, delta, noise)
    return _cases[key]


def test_path_taken(engine, oracle):
    """Fails without the feature: at (20, 200, f = 6), k = 1, with 19 rows
    added, one more fused launch and no border launch; the timing table shows
    k_small once, no noise kernel, none of the chain's kernels and no copy."""
    X, delta, noise = _case(oracle, 20, 200, 1)
    arr = _Arrival(delta, noise, _lib.BK_HOST)
    ref, rs, rrow = _two_calls(engine, X, 19, arr, f=6)
    assert rs == TWO_SMALL, rs
    noise_name = _lib.lib().bk_kernel_name(BK_K_NOISE).decode()
    _begin(engine, X, 19)
    s0 = engine.collect_stats()
    engine.timing_enable(True)
    slot, sel, sc, mean = arr.add_finish(engine, 200, f=6)
    t = engine.timing_read()
    engine.timing_enable(False)
    assert slot == 19
    assert _delta(engine.collect_stats(), s0) == FUSED
    assert ONE in t and t[ONE]["count"] == 1, t
    assert not any(k in t for k in CHAIN + (noise_name, "k_mean", "d2h", "h2d")), t
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref, "fused")
    assert _same_bits(engine.collect_read_rows([19])[0], rrow)
    # the small path off: the noise kernel, the border and the chain, the same bits
    engine.set_small_path(False)
    try:
        _begin(engine, X, 19)
        s0 = engine.collect_stats()
        engine.timing_enable(True)
        slot, sel, sc, mean = arr.add_finish(engine, 200, f=6)
        t = engine.timing_read()
        engine.timing_enable(False)
        off = ((sel, sc, mean), _record(engine))
    finally:
        engine.set_small_path(True)
    assert _delta(engine.collect_stats(), s0) == TWO_CHAIN
    assert ONE not in t and noise_name in t and all(k in t for k in CHAIN), t
    _assert_bitwise(off, ref, "small path off")


# j = 1: the second-ever arrival (n = 2, f = 1); j = 127: the 128-row edge; d =
# 201: the lone last column and the pad column; d = 32,768: the 32-chunk edge
# (n = 8 there); k = 9 crosses the 8-deep unroll, k = 64 is the cap
@pytest.mark.parametrize("k,d,j", [
    (1, 25, 1), (1, 200, 19), (1, 201, 127), (1, 7850, 19), (1, 32768, 7),
    (2, 25, 127), (2, 201, 19), (2, 7850, 127), (2, 200, 1),
    (9, 201, 1), (9, 25, 19), (9, 7850, 19), (9, 32768, 7), (9, 200, 127),
    (64, 201, 19), (64, 25, 1), (64, 200, 127), (64, 7850, 1), (64, 32768, 7)])
def test_bitwise_against_add_noised_then_finish(engine, oracle, k, d, j):
    n = j + 1
    f = {2: 1, 8: 2, 20: 6, 128: 38}[n]
    X, delta, noise = _case(oracle, n, d, k)
    for where in WHERES:
        arr = _Arrival(delta, noise, where)
        got, _, rs, _ = _both(engine, X, j, arr, (k, d, j, where), path=_path(where, d, k), f=f)
        assert rs == TWO_SMALL, rs
        assert int(got[1][6]) == d and int(got[1][7]) == max(0, n - f - 2)


def test_orders_and_outputs(engine, oracle):
    n, d, f = 60, 777, 18
    X, delta, noise = _case(oracle, n, d, 2)
    rng = np.random.default_rng(8)
    perm = rng.permutation(n).astype(np.int64)
    with_new = np.concatenate([rng.choice(n - 1, size=20, replace=False), [n - 1]]).astype(np.int64)
    rng.shuffle(with_new)
    without = rng.choice(n - 1, size=21, replace=False).astype(np.int64)
    for where in WHERES:
        arr = _Arrival(delta, noise, where)
        _both(engine, X, n - 1, arr, "null order", f=f)
        _both(engine, X, n - 1, arr, "permutation", order=perm, f=f)
        _both(engine, X, n - 1, arr, "subset with the new slot", order=with_new, f=6)
        _both(engine, X, n - 1, arr, "subset without the new slot", order=without, f=6)
        # ... whose row and border were written all the same: a finish over every row
        after = _finish(engine, f=f)
        _two_calls(engine, X, n - 1, arr, order=without, f=6)
        _assert_bitwise(after, _finish(engine, f=f), "all rows after the subset")
    arr = _Arrival(delta, noise, _lib.BK_HOST)
    for sc in (True, False):
        for mean in (True, False):
            got, _, _, _ = _both(engine, X, n - 1, arr, ("outputs", sc, mean), order=perm, f=f,
                                 want_scores=sc, want_mean=mean)
            assert (got[0][1] is None) == (not sc) and (got[0][2] is None) == (not mean)


def test_stored_row_special_values(engine, oracle):
    """-0.0 in the delta and in every noise vector stores +0.0 (the sum starts
    from 0.0); a NaN and an inf in the noise give the reference's NaN / inf
    pattern in the stored row and in the scores"""
    n, d, k = 20, 201, 3
    X, delta, noise = _case(oracle, n, d, k)
    dz, nz = delta.copy(), noise.copy()
    cols = [0, 1, 64, 199, 200]  # both halves of a pair, and the lone last column
    dz[cols] = -0.0
    nz[:, cols] = -0.0
    for where in WHERES:
        arr = _Arrival(dz, nz, where)
        _, _, _, row = _both(engine, X, n - 1, arr, ("-0.0", where), f=6)
        assert np.array_equal(_bits(row[cols]), np.zeros(len(cols), np.int64)), row[cols]
    nb = noise.copy()
    nb[1, 5] = np.nan
    nb[2, 200] = np.inf
    nb[0, 64] = -np.inf
    for where in WHERES:
        arr = _Arrival(delta, nb, where)
        got, ref, _, row = _both(engine, X, n - 1, arr, ("nan / inf", where), f=6)
        assert np.isnan(row[5]) and row[200] == np.inf and row[64] == -np.inf
        assert np.array_equal(np.isnan(got[0][1]), np.isnan(ref[0][1]))
        assert np.array_equal(np.isinf(got[0][1]), np.isinf(ref[0][1]))
        assert not np.isfinite(got[0][1][n - 1])


def _later(engine, X, j):
    """what later calls see of a collection whose row j arrived: a plain add, a
    finish, a batched finish of two orders, and the rows read back"""
    out = []
    assert engine.collect_add(X[j + 1]) == j + 1
    out.append(_finish(engine, f=j // 3))
    rng = np.random.default_rng(j)
    orders = np.stack([np.concatenate([rng.choice(j, size=11, replace=False), [j]])
                       for _ in range(2)]).astype(np.int64)
    batch = engine.collect_finish_batch(orders, 4)
    rows = engine.collect_read_rows([j, j + 1, 0])
    return out, batch, rows


def test_state_afterwards(engine, oracle):
    n, d, j, k = 45, 1500, 40, 2
    X, _, noise = _case(oracle, n, d, k)
    delta = np.ascontiguousarray(X[j])
    for where in WHERES:
        arr = _Arrival(delta, noise, where)
        _two_calls(engine, X, j, arr, n_cap=n, f=13)
        want, wbatch, wrows = _later(engine, X, j)
        _, gs, _ = _fused(engine, X, j, arr, n_cap=n, f=13)
        assert gs == FUSED
        got, gbatch, grows = _later(engine, X, j)
        _assert_bitwise(got[0], want[0], ("later finish", where))
        assert np.array_equal(gbatch[0], wbatch[0])
        assert _same_bits(gbatch[1], wbatch[1]) and _same_bits(gbatch[2], wbatch[2])
        assert _same_bits(grows, wrows)


def test_k0_is_add_finish(engine, oracle):
    n, d = 20, 200
    X, delta, _ = _case(oracle, n, d, 1)
    _begin(engine, X, n - 1)
    s0 = engine.collect_stats()
    slot, sel, sc, mean = engine.collect_add_finish(delta, f=6)
    ref = ((sel, sc, mean), _record(engine))
    assert _delta(engine.collect_stats(), s0) == FUSED
    rrow = engine.collect_read_rows([n - 1])[0]
    arr = _Arrival(delta, np.empty((0, d)), _lib.BK_HOST)
    got, gs, grow = _fused(engine, X, n - 1, arr, f=6)
    assert gs == FUSED  # fused_arrivals + 1: k_collect_arrive, as collect_add_finish
    _assert_bitwise(got, ref, "k = 0")
    assert np.array_equal(_bits(grow), _bits(rrow)) and np.array_equal(_bits(grow), _bits(delta))
    # the Engine's array form: noise None
    _begin(engine, X, n - 1)
    slot, sel, sc, mean = engine.collect_add_noised_finish(delta, None, f=6)
    _assert_bitwise(((sel, sc, mean), _record(engine)), ref, "noise None")


def test_fallbacks_same_bits(engine, oracle):
    """outside the fused range the call is the noised add and then the finish"""
    # 129 rows after the add; a finish of 100 of them is the one-launch finish
    X, delta, noise = _case(oracle, 129, 40, 2)
    sub = np.concatenate([np.random.default_rng(2).choice(128, size=99, replace=False),
                          [128]]).astype(np.int64)
    for where in WHERES:
        arr = _Arrival(delta, noise, where)
        _both(engine, X, 128, arr, "129 rows collected", path=TWO_SMALL, order=sub, f=30)
    _both(engine, X, 128, arr, "n = 129", path=TWO_CHAIN, f=40)
    # host rows of more than 32 KiB but pinned ones with k = 1: measured no
    # faster fused, the two calls (device rows and pinned k = 1: the launch)
    W, dw, nw = _case(oracle, 100, 7850, 2)
    for where, k, path in ((_lib.BK_HOST, 1, TWO_SMALL), (_lib.BK_HOST, 2, TWO_SMALL),
                           (_lib.BK_HOST_PINNED, 2, TWO_SMALL), (_lib.BK_HOST_PINNED, 1, FUSED),
                           (_lib.BK_DEVICE, 2, FUSED)):
        assert _path(where, 7850, k) == path
        _both(engine, W, 99, _Arrival(dw, nw[:k], where), ("100 x 7,850", where, k), path=path, f=30)
    # d past k_collect_small's cap: the chain, or with the wide path on its launch
    Z, dz, nz = _case(oracle, 5, 32769, 1)
    for where in WHERES:
        arr = _Arrival(dz, nz, where)
        _both(engine, Z, 4, arr, "d = 32,769", path=TWO_CHAIN, f=1)
    engine.set_collect_wide(True)
    try:
        _both(engine, Z, 4, arr, "d = 32,769, wide", path=TWO_SMALL, f=1)
    finally:
        engine.set_collect_wide(False)


def test_array_form(engine, oracle):
    """Engine.collect_add_noised_finish on numpy arrays: a vector (k = 1) and a
    (k, d) array, against collect_add_noised + collect_finish"""
    n, d = 20, 201
    X, delta, noise = _case(oracle, n, d, 3)
    for nz in (noise[0], noise):
        _begin(engine, X, n - 1)
        assert engine.collect_add_noised(delta, nz) == n - 1
        ref = _finish(engine, f=6)
        rrow = engine.collect_read_rows([n - 1])[0]
        _begin(engine, X, n - 1)
        s0 = engine.collect_stats()
        slot, sel, sc, mean = engine.collect_add_noised_finish(delta, nz, f=6)
        assert slot == n - 1 and _delta(engine.collect_stats(), s0) == FUSED
        _assert_bitwise(((sel, sc, mean), _record(engine)), ref, "array form")
        assert _same_bits(engine.collect_read_rows([n - 1])[0], rrow)


def test_errors_leave_the_collection(engine, oracle):
    n, d, f = 12, 64, 3
    X, delta, noise = _case(oracle, n + 1, d, 2)
    L = _lib.lib()
    sel = np.empty(n + 1, np.int64)
    row = np.ascontiguousarray(delta)
    v0, v1 = np.ascontiguousarray(noise[0]), np.ascontiguousarray(noise[1])
    nzp = (ctypes.c_void_p * 2)(v0.ctypes.data, v1.ctypes.data)
    hole = (ctypes.c_void_p * 2)(v0.ctypes.data, None)
    many = (ctypes.c_void_p * 65)(*([v0.ctypes.data] * 65))

    def call(ctx, dp, nz, k, where, order, nn, ff, selp=sel.ctypes.data):
        o = np.ascontiguousarray(order, dtype=np.int64) if order is not None else None
        return L.bk_collect_add_noised_finish(ctx, dp, nz, k, where,
                                              o.ctypes.data if o is not None else None, nn, ff,
                                              None, selp, None, None, None)

    fresh = Engine(0)  # no begin on this context
    try:
        assert call(fresh.ctx, row.ctypes.data, nzp, 2, _lib.BK_HOST, None, 2, 1) == _lib.BK_EINVAL
        assert "bk_collect_add_noised without bk_collect_begin" in _lib.last_error()
        # the checks that need no collection come first, ENOTSUP and sel_idx among them
        assert call(fresh.ctx, row.ctypes.data, many, 65, _lib.BK_HOST, None, 2, 1) == _lib.BK_ENOTSUP
        assert call(fresh.ctx, row.ctypes.data, nzp, 2, _lib.BK_HOST, None, 2, 1,
                    selp=None) == _lib.BK_EINVAL
        assert "null sel_idx" in _lib.last_error()
        fresh.collect_begin(4, d, np.float32)
        assert call(fresh.ctx, row.ctypes.data, nzp, 2, _lib.BK_HOST, None, 1, 1) == _lib.BK_EINVAL
        assert "BK_F32" in _lib.last_error()
        # a first-ever arrival cannot finish: n = 1 leaves no f
        fresh.collect_begin(4, d)
        assert call(fresh.ctx, row.ctypes.data, nzp, 2, _lib.BK_HOST, None, 1, 1) == _lib.BK_EINVAL
        assert fresh.collect_count() == 0
    finally:
        fresh.close()

    _begin(engine, X, n, n_cap=n + 1)
    ref = _finish(engine, f=f)
    s0 = engine.collect_stats()
    H, E, U = _lib.BK_HOST, _lib.BK_EINVAL, _lib.BK_ENOTSUP
    rp = row.ctypes.data
    bad = [  # in the documented order: each call has every later fault too, or none
        (None, None, -1, 7, None, 0, 0, None, E, "null delta"),
        (rp, None, -1, 7, None, 0, 0, None, E, "need k >= 0"),
        (rp, None, 2, 7, None, 0, 0, None, E, "null noises with k=2"),
        (rp, many, 65, 7, None, 0, 0, None, E, "bad where"),
        (rp, many, 65, H, None, 0, 0, None, U, "BK_COLLECT_NOISE_MAX_K"),
        (rp, hole, 2, H, None, 0, 0, None, E, "null sel_idx"),
        (rp, hole, 2, H, None, 0, 0, sel.ctypes.data, E, "null noise vector (0, 1)"),
        (rp, nzp, 2, H, [0, 1, n + 1], 3, 1, sel.ctypes.data, E, "no collected slot"),
        (rp, nzp, 2, H, [-1, 1, 2], 3, 1, sel.ctypes.data, E, "no collected slot"),
        (rp, nzp, 2, H, [0, n, 0], 3, 1, sel.ctypes.data, E, "repeats a slot"),
        (rp, nzp, 2, H, None, n, f, sel.ctypes.data, E, "a null order needs"),
        (rp, nzp, 2, H, None, n + 2, f, sel.ctypes.data, E, "rows collected"),
        (rp, nzp, 2, H, None, n + 1, 0, sel.ctypes.data, E, "need 1 <= f < n"),
        (rp, nzp, 2, H, None, n + 1, n + 1, sel.ctypes.data, E, "need 1 <= f < n"),
    ]
    for dp, nz, k, where, order, nn, ff, selp, status, word in bad:
        assert call(engine.ctx, dp, nz, k, where, order, nn, ff, selp=selp) == status, word
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert engine.collect_count() == n
    assert engine.collect_stats() == s0
    _assert_bitwise(_finish(engine, f=f), ref, "after the refused calls")
    # the new slot is a collected slot for the order: n names it
    slot, s, _, _ = engine.collect_add_noised_finish(row, noise, order=[n, 0, 5], f=1)
    assert slot == n and engine.collect_count() == n + 1
    # past n_cap (before a null noise vector is looked for)
    assert call(engine.ctx, rp, hole, 2, H, None, n + 2, f) == E
    assert "bk_collect_add_noised" in _lib.last_error() and "past n_cap" in _lib.last_error()
    assert engine.collect_count() == n + 1


def test_krum_validator_noised_last(engine, oracle):
    """KRUMValidator(collect=True, noised=True): add_update(..., last=True) on
    the 20th update against last=False and compute_scores()"""
    n, d = 20, 200
    X, _, _ = _case(oracle, n, d, 1)
    rng = np.random.default_rng(5)
    Nz = 1e-2 * rng.standard_normal((n, d))
    ids = [7 + 3 * i for i in range(n)]
    arrival = [int(i) for i in rng.permutation(n)]

    def feed(v, last):
        for q, i in enumerate(arrival):
            # (one update without Noise: k = 0)
            u = Update(SourceID=ids[i], Delta=X[i].copy(), Noise=None if i == arrival[0] else Nz[i].copy())
            v.add_update(u, last=last and q == n - 1)

    two = KRUMValidator(engine=engine, collect=True, noised=True, n_cap=n).initialize()
    feed(two, False)
    two.compute_scores()
    two_last = two.noised_delta(n - 1).copy()
    two_rows = [two.noised_delta(i).copy() for i in range(n)]
    one = KRUMValidator(engine=engine, collect=True, noised=True, n_cap=n).initialize()
    feed(one, True)
    assert engine.collect_stats()["fused_arrivals"] == 1
    assert [u.SourceID for u in one.UpdateList] == sorted(ids)
    assert one.AcceptedList == two.AcceptedList and len(one.AcceptedList) == n - n // 2
    assert np.array_equal(_bits(one.noised_delta(n - 1)), _bits(two_last))
    # the last arrival's row, wherever the sort by SourceID put it
    at = [u.SourceID for u in one.UpdateList].index(ids[arrival[-1]])
    assert np.array_equal(_bits(one.noised_delta(at)), _bits(two_rows[at]))
