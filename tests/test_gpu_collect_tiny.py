"""The tiny collection (bk_set_collect_tiny, bk_collect_tiny.hip): at most 16
rows collected, d <= 128, every add, finish and fused arrival ONE launch of one
workgroup (k_collect_tiny) with no copy call.

The bar: collect_tiny_stats(), collect_stats() and the timing table show the
path taken; every output -- sel, scores, mean, the eight margin fields, the
stored rows and whatever later calls give -- is BITWISE what the same sequence
of calls gives on the same engine with the switch off (the reference of every
check here: a second pass, never the tiny path itself), and the chain's."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import golden_util as GU  # noqa: E402
from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import Engine, KRUMValidator, Update  # noqa: E402

ONE = "k_small"
H, P, D = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
WHERES = (H, P, D)
ZERO4 = {"border": 0, "border_reduce": 0, "one_launch_finishes": 0, "fused_arrivals": 0}
ZERO3 = {"adds": 0, "finishes": 0, "arrivals": 0}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _record(engine):
    """the eight public margin fields of the last call, raw"""
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _assert_same(got, ref, what):
    """bitwise, a NaN matching a NaN (its payload apart); nested tuples alike"""
    if isinstance(ref, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(ref), what
        for i, (g, r) in enumerate(zip(got, ref)):
            _assert_same(g, r, (what, i))
    elif ref is None:
        assert got is None, what
    elif isinstance(ref, np.ndarray) and ref.dtype.kind == "f":
        assert got.shape == ref.shape, what
        nan = np.isnan(ref)
        assert np.array_equal(nan, np.isnan(got)), (what, got, ref)
        assert np.array_equal(_bits(got[~nan]), _bits(ref[~nan])), (what, got, ref)
    else:
        assert np.array_equal(got, ref), (what, got, ref)


class _Src:
    """the rows of X in `where` memory, every row 8 bytes past a 16-byte
    boundary (8-byte but not 16-byte aligned), and their pointers"""

    def __init__(self, X, where):
        X = np.ascontiguousarray(X)
        self.where, self.X = where, X
        n, d = X.shape
        self.pitch = (d * X.itemsize + 15) // 16 * 16 + 16
        total = n * self.pitch + 32
        if where == H:
            self.buf = np.empty(total, np.uint8)
            base, img = self.buf.ctypes.data, self.buf
        elif where == P:
            self.buf = torch.empty(total, dtype=torch.uint8).pin_memory()
            base, img = self.buf.data_ptr(), self.buf.numpy()
        else:
            self.buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            base, img = self.buf.data_ptr(), np.zeros(total, np.uint8)
        off = (-base) % 16 + 8
        for i in range(n):
            at = off + i * self.pitch
            img[at:at + d * X.itemsize] = X[i].view(np.uint8)
        if where == D:
            self.buf.copy_(torch.from_numpy(img))
            torch.cuda.synchronize()
        self.base = base + off
        assert self.ptr(0) % 16 == 8

    def ptr(self, i):
        return self.base + i * self.pitch

    def ptrs(self, i, cnt):
        return (ctypes.c_void_p * cnt)(*[self.ptr(r) for r in range(i, i + cnt)])


def _tiny_arrival(d, dtype):
    """a fused arrival takes the tiny launch up to 512-byte rows; longer ones were
    not ahead of today's fused launch at the one shape measured (16 x 128 fp64)
    and take that inside the entry -- but for the noised form from host rows"""
    return d * np.dtype(dtype).itemsize <= 512


def _finish(engine, **kw):
    return engine.collect_finish(**kw), _record(engine)


def _add_finish(engine, src, i, d, order=None, n=None, f=None, want_scores=True, want_mean=True):
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int64)
        n = len(order)
    elif n is None:
        n = engine.collect_count() + 1
    sel = np.empty(n - f, np.int64)
    sc = np.empty(n) if want_scores else None
    mean = np.empty(d) if want_mean else None
    slot, m = engine.collect_add_finish_ptr(
        src.ptr(i), src.where, order.ctypes.data if order is not None else None, n, f,
        sel.ctypes.data, sc.ctypes.data if sc is not None else None,
        mean.ctypes.data if mean is not None else None)
    assert slot == i and m == n - f
    return (sel, sc, mean), _record(engine)


def _rows(engine, n, dtype):
    """the stored rows (fp64 collections: bk_collect_read_rows is fp64 only)"""
    return engine.collect_read_rows(np.arange(n)) if dtype == np.float64 else None


def _arrivals(engine, X, f, where=H, groups=None, n_cap=None, **kw):
    """rows 0..n-2 arrive (one at a time, or in `groups`), the last through
    add_finish; then a plain finish and the stored rows"""
    n, d = X.shape
    src = _Src(X, where)
    engine.collect_begin(n_cap or n, d, X.dtype)
    i = 0
    for g in groups or [1] * (n - 1):
        assert engine.collect_add_ptr(src.ptrs(i, g), g, where) == i
        i += g
    assert i == n - 1
    out = [_add_finish(engine, src, n - 1, d, f=f, **kw)]
    out.append(_finish(engine, f=f))
    out.append(_rows(engine, n, X.dtype))
    return out


def _onoff(engine, scenario, what, chain=False):
    """the scenario with the switch off (THE REFERENCE), then on -> the tiny
    pass's outputs, its tiny stats and collect stats; chain: also against the
    small path off"""
    engine.set_collect_tiny(False)
    ref = scenario(engine)
    assert engine.collect_tiny_stats() == ZERO3, what
    engine.set_collect_tiny(True)
    try:
        got = scenario(engine)
        ts, cs = engine.collect_tiny_stats(), engine.collect_stats()
        _assert_same(got, ref, what)
        if chain:
            engine.set_small_path(False)
            try:
                off = scenario(engine)
                assert engine.collect_tiny_stats() == ZERO3, what
            finally:
                engine.set_small_path(True)
            _assert_same(off, ref, (what, "chain"))
    finally:
        engine.set_collect_tiny(False)
    return got, ts, cs


def test_path_taken(engine, oracle):
    """Fails without the feature.  Config A's shape: nine adds, the fused last
    arrival and a finish are eleven k_collect_tiny launches, one BK_K_SMALL entry
    per call, no border launch, no copy and no noise kernel in the timing table"""
    X = oracle.synth(10, 25, 41, 2)

    def timed_run(e):
        e.timing_enable(True)
        try:
            out = _arrivals(e, X, 2)
            return out, e.timing_read()
        finally:
            e.timing_enable(False)

    times = []

    def scenario(e):
        out, t = timed_run(e)
        times.append(t)
        return out

    _, ts, cs = _onoff(engine, scenario, "config A shape", chain=True)
    assert ts == {"adds": 9, "finishes": 1, "arrivals": 1}, ts
    assert cs == {"border": 0, "border_reduce": 0, "one_launch_finishes": 1, "fused_arrivals": 1}, cs
    t_off, t_on, t_chain = times
    assert set(t_on) == {ONE} and t_on[ONE]["count"] == 11, t_on
    assert "h2d" not in t_on and "d2h" not in t_on and "k_noise" not in t_on
    assert t_off[ONE]["count"] == 2, t_off  # today: the fused arrival and the finish
    assert ONE not in t_chain, t_chain


@pytest.mark.parametrize("name", ["A_creditcard", "A_n4_k0_tie"])
def test_goldens(name, engine, oracle):
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X, dtype=np.float64)
    got, ts, _ = _onoff(engine, lambda e: _arrivals(e, X, p["f"]), name, chain=True)
    assert np.array_equal(got[0][0][0], GU.load(name)["sel"]), name
    assert np.array_equal(got[1][0][0], GU.load(name)["sel"]), name
    assert ts == {"adds": X.shape[0] - 1, "finishes": 1, "arrivals": 1}


# the full range in both dtypes; odd d and the pad columns; m = 1 with k <= 0
@pytest.mark.parametrize("n,d,f,dtype", [
    (16, 128, 4, np.float64), (16, 128, 4, np.float32), (16, 127, 5, np.float64),
    (16, 127, 5, np.float32), (5, 1, 1, np.float64), (5, 1, 2, np.float32),
    (2, 3, 1, np.float64), (2, 3, 1, np.float32), (3, 2, 1, np.float64),
    (16, 64, 4, np.float64), (16, 65, 4, np.float64)])  # either side of the fused arrival's cut
def test_range_edges(engine, oracle, n, d, f, dtype):
    X = oracle.synth(n, d, 500 + n + d, max(1, n // 4), dtype=dtype)
    got, ts, cs = _onoff(engine, lambda e: _arrivals(e, X, f), (n, d, f, dtype), chain=True)
    tiny = _tiny_arrival(d, dtype)
    assert ts == {"adds": n - 1, "finishes": 1, "arrivals": 1 if tiny else 0}
    assert cs == {"border": 0, "border_reduce": 0, "one_launch_finishes": 1, "fused_arrivals": 1}
    rec = got[0][1]
    assert int(rec[6]) == d and int(rec[7]) == max(0, n - f - 2)


def _special(name, oracle):
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X, dtype=np.float64)
    rows = list(range(12)) + [17, 30, 12, 13] if name == "dup_rows" else list(range(16))
    return np.ascontiguousarray(X[rows, :128])


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows"])
def test_special_values(name, engine, oracle):
    """the special-value goldens' rows, cut to 16 x 128; the special row arrives last too"""
    X = _special(name, oracle)
    if name == "dup_rows":
        assert np.array_equal(X[3], X[12]) and np.array_equal(X[9], X[13])
    else:
        assert not np.isfinite(X).all()
    bad = np.flatnonzero(~np.isfinite(X).all(axis=1))
    sp = int(bad[0]) if bad.size else 12
    arrive = [r for r in range(16) if r != sp] + [sp]
    # (16 x 64: the fused arrival is the tiny launch's too)
    for A in (X, np.ascontiguousarray(X[arrive]), np.ascontiguousarray(X[arrive][:, :64])):
        _, ts, _ = _onoff(engine, lambda e: _arrivals(e, A, 4), name, chain=True)
        assert ts == {"adds": 15, "finishes": 1, "arrivals": 1 if A.shape[1] == 64 else 0}


def test_orders_and_finishes(engine, oracle):
    n, d = 16, 25
    X = oracle.synth(n, d, 61, 4)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n).astype(np.int64)
    sub7 = np.concatenate([rng.choice(n - 1, size=6, replace=False), [n - 1]]).astype(np.int64)
    rng.shuffle(sub7)
    without = rng.choice(n - 1, size=7, replace=False).astype(np.int64)

    def scenario(e):
        out = []
        for kw in (dict(f=4), dict(order=perm, f=4), dict(order=sub7, f=2),
                   dict(order=without, f=2),
                   dict(order=perm, f=4, want_scores=False),
                   dict(order=sub7, f=2, want_mean=False),
                   dict(f=4, want_scores=False, want_mean=False)):
            src = _Src(X, H)
            e.collect_begin(n, d)
            assert e.collect_add_ptr(src.ptrs(0, n - 1), n - 1, H) == 0
            out.append(_add_finish(e, src, n - 1, d, **kw))
            # the row and its border were written whether the order named it or not
            a, b = _finish(e, f=4), _finish(e, f=4)
            _assert_same(b, a, "finish twice")
            out += [a, _finish(e, order=sub7, f=2), _finish(e, order=perm, f=5, want_mean=False),
                    _finish(e, order=without, f=3, want_scores=False), _rows(e, n, np.float64)]
        return out

    _onoff(engine, scenario, "orders", chain=True)


def test_sources_and_counts(engine, oracle):
    """pageable rows off 16-byte alignment, pinned rows, device rows at an 8-byte
    but not 16-byte aligned address; adds of 1, 3 and 16 rows in one call"""
    for dtype in (np.float64, np.float32):
        X = oracle.synth(16, 25, 62, 4, dtype=dtype)
        ref = None
        for where in WHERES:
            for groups in ([1] * 15, [3, 1, 3, 8], [15]):
                got, ts, _ = _onoff(engine, lambda e: _arrivals(e, X, 4, where=where, groups=groups),
                                    (dtype, where, groups))
                assert ts == {"adds": len(groups), "finishes": 1, "arrivals": 1}
                ref = ref or got
                _assert_same(got, ref, ("whatever the source and the grouping", where, groups))

    def sixteen(e):  # 16 rows in one add, then a finish
        X64 = oracle.synth(16, 128, 63, 4)
        src = _Src(X64, D)
        e.collect_begin(40, 128)
        assert e.collect_add_ptr(src.ptrs(0, 16), 16, D) == 0
        return [_finish(e, f=4), _rows(e, 16, np.float64)]

    _, ts, _ = _onoff(engine, sixteen, "16 rows in one add")
    assert ts == {"adds": 1, "finishes": 1, "arrivals": 0}


class _Noised:
    """n updates as deltas and k noise vectors each, in `where` memory"""

    def __init__(self, delta, noise, where):
        self.n, self.d = delta.shape
        self.k, self.where = noise.shape[1], where
        self.ds = _Src(delta, where)
        self.ns = _Src(noise.reshape(self.n * self.k, self.d), where) if self.k else None

    def nz(self, i, cnt=1):
        return self.ns.ptrs(i * self.k, cnt * self.k) if self.k else None

    def add(self, e, i, cnt=1):
        return e.collect_add_noised_ptr(self.ds.ptrs(i, cnt), self.nz(i, cnt), self.k, cnt, self.where)

    def add_finish(self, e, i, f):
        n = e.collect_count() + 1
        sel, sc, mean = np.empty(n - f, np.int64), np.empty(n), np.empty(self.d)
        slot, m = e.collect_add_noised_finish_ptr(self.ds.ptr(i), self.nz(i), self.k, self.where, None,
                                                  n, f, sel.ctypes.data, sc.ctypes.data,
                                                  mean.ctypes.data)
        assert slot == i and m == n - f
        return (sel, sc, mean), _record(e)


_noise_cases = {}


def _noise_case(n, d, k):
    if (n, d, k) not in _noise_cases:
        rng = np.random.default_rng(11 * n + 5 * d + k)
        delta = rng.standard_normal((n, d))
        noise = 1e-2 * rng.standard_normal((n, k, d))
        delta[1, 0] = -0.0
        noise[1, :, 0] = -0.0
        _noise_cases[(n, d, k)] = (delta, noise)
    return _noise_cases[(n, d, k)]


@pytest.mark.parametrize("k", [0, 1, 2, 64])
def test_noised(engine, oracle, k):
    """host and device vectors; plain and noised adds mixed; the stored rows
    bitwise bk_noise_apply_device's"""
    n, d, f = 6, 27, 2
    delta, noise = _noise_case(n, d, k)
    want = delta
    if k:
        tD, tN = torch.from_numpy(delta).cuda(), torch.from_numpy(noise).cuda()
        out = torch.empty((n, d), dtype=torch.float64, device="cuda")
        # the k vectors of row i at noise[i, j]: one call per row (noise_ld = d)
        for i in range(n):
            engine.noise_apply_ptr(tD[i].data_ptr(), 1, d, d, tN[i].data_ptr(), k, d,
                                   out[i].data_ptr(), d)
        engine.synchronize()
        want = out.cpu().numpy()
    plain = _Src(want, H)
    for where in WHERES:
        nz = _Noised(delta, noise, where)

        def scenario(e):
            e.collect_begin(n, d)
            assert nz.add(e, 0) == 0
            assert nz.add(e, 1, 2) == 1  # two updates in one call
            assert e.collect_add_ptr(plain.ptrs(3, 1), 1, H) == 3  # a plain add in between
            assert nz.add(e, 4) == 4
            return [nz.add_finish(e, 5, f), _finish(e, f=f), _rows(e, n, np.float64)]

        got, ts, cs = _onoff(engine, scenario, (k, where), chain=True)
        # (a noised add is one launch per update, a plain one -- k = 0 -- one per call)
        assert ts == {"adds": 5 if k else 4, "finishes": 1, "arrivals": 1}, ts
        assert cs["border"] == cs["border_reduce"] == 0
        assert np.array_equal(_bits(got[2]), _bits(want)), (k, where)


def test_noised_path(engine, oracle):
    """one BK_K_SMALL entry per call and no noise kernel, no copy"""
    n, d, k, f = 4, 25, 2, 2
    delta, noise = _noise_case(n, d, k)
    nz = _Noised(delta, noise, H)
    engine.set_collect_tiny(True)
    try:
        engine.collect_begin(n, d)
        engine.timing_enable(True)
        for i in range(n - 1):
            assert nz.add(engine, i) == i
        nz.add_finish(engine, n - 1, f)
        t = engine.timing_read()
        engine.timing_enable(False)
        assert set(t) == {ONE} and t[ONE]["count"] == n, t
        assert engine.collect_tiny_stats() == {"adds": n - 1, "finishes": 0, "arrivals": 1}
    finally:
        engine.timing_enable(False)
        engine.set_collect_tiny(False)


def test_leaving_the_range(engine, oracle):
    # d = 129: today's paths, the tiny stats stay put
    X = oracle.synth(6, 129, 64, 1)
    _, ts, cs = _onoff(engine, lambda e: _arrivals(e, X, 2), "d = 129")
    assert ts == ZERO3 and cs["border"] == 5 and cs["fused_arrivals"] == 1

    # the 17th arrival of the same collection, and later ones
    Y = oracle.synth(19, 25, 65, 4)

    def seventeen(e):
        src = _Src(Y, H)
        e.collect_begin(19, 25)
        for i in range(16):
            assert e.collect_add_ptr(src.ptrs(i, 1), 1, H) == i
        out = [_finish(e, f=4)]
        seen = (e.collect_tiny_stats(), e.collect_stats())
        assert e.collect_add_ptr(src.ptrs(16, 1), 1, H) == 16
        out.append(_finish(e, f=5))
        out.append(_finish(e, order=np.arange(3, 12), f=3))  # 9 of 17 collected: not tiny
        out.append(_add_finish(e, src, 17, 25, f=5))
        out.append(_rows(e, 18, np.float64))
        stats.append((seen, e.collect_tiny_stats(), e.collect_stats()))
        return out

    stats = []
    _onoff(engine, seventeen, "17th arrival")
    (ts16, cs16), ts, cs = stats[1]
    assert ts16 == {"adds": 16, "finishes": 1, "arrivals": 0} and ts == ts16
    assert cs16 == {"border": 0, "border_reduce": 0, "one_launch_finishes": 1, "fused_arrivals": 0}
    assert cs == {"border": 1, "border_reduce": 1, "one_launch_finishes": 3, "fused_arrivals": 1}

    # 16 tiny arrivals, then the switch off, then the batched and ragged finishes
    Z = oracle.synth(16, 100, 66, 4)
    rng = np.random.default_rng(9)
    orders = np.stack([rng.permutation(16)[:9] for _ in range(3)]).astype(np.int64)
    ragged = [rng.permutation(16)[:m].astype(np.int64) for m in (16, 5, 9, 5)]

    def batched(e, tiny):
        src = _Src(Z, P)
        e.set_collect_tiny(tiny)
        try:
            e.collect_begin(16, 100)
            for i in range(16):
                assert e.collect_add_ptr(src.ptrs(i, 1), 1, P) == i
            assert e.collect_tiny_stats()["adds"] == (16 if tiny else 0)
        finally:
            e.set_collect_tiny(False)
        return [e.collect_finish_batch(orders, 3), e.collect_finish_ragged(ragged, [4, 1, 2, 2]),
                _rows(e, 16, np.float64)]

    _assert_same(batched(engine, True), batched(engine, False), "batched and ragged finishes")


def test_small_path_off_and_default(engine, oracle):
    """the switch is off by default; the small path off disables it"""
    X = oracle.synth(4, 25, 67, 1)
    fresh = Engine(0)
    try:
        _arrivals(fresh, X, 2)
        assert fresh.collect_tiny_stats() == ZERO3
        assert fresh.collect_stats()["border"] == 3
        fresh.set_collect_tiny(True)
        fresh.set_small_path(False)
        _arrivals(fresh, X, 2)
        assert fresh.collect_tiny_stats() == ZERO3
        fresh.set_small_path(True)
        _arrivals(fresh, X, 2)
        assert fresh.collect_tiny_stats() == {"adds": 3, "finishes": 1, "arrivals": 1}
    finally:
        fresh.close()


def test_errors_leave_the_collection(engine, oracle):
    n, d, f = 7, 25, 2
    X = oracle.synth(n + 1, d, 68, 1)
    L = _lib.lib()
    sel = np.empty(n + 1, np.int64)
    row = np.ascontiguousarray(X[n])
    v0 = np.ascontiguousarray(X[0])
    one = (ctypes.c_void_p * 1)(row.ctypes.data)
    null1 = (ctypes.c_void_p * 1)(None)
    nzp = (ctypes.c_void_p * 2)(v0.ctypes.data, v0.ctypes.data)
    many = (ctypes.c_void_p * 65)(*([v0.ctypes.data] * 65))
    two = (ctypes.c_void_p * 2)(row.ctypes.data, row.ctypes.data)
    rp, sp = row.ctypes.data, sel.ctypes.data
    E, U = _lib.BK_EINVAL, _lib.BK_ENOTSUP
    first = ctypes.c_int64(-7)

    def order(o):
        return np.ascontiguousarray(o, dtype=np.int64)

    bad3, rep3 = order([0, 1, n + 1]), order([0, n, 0])
    engine.set_collect_tiny(True)
    try:
        src = _Src(X, H)
        engine.collect_begin(n + 1, d)
        assert engine.collect_add_ptr(src.ptrs(0, n), n, H) == 0
        ref = _finish(engine, f=f)
        t0, s0 = engine.collect_tiny_stats(), engine.collect_stats()
        bad = [
            (lambda: L.bk_collect_add(engine.ctx, null1, 1, H, ctypes.byref(first)), E, "null row 0"),
            (lambda: L.bk_collect_add(engine.ctx, two, 2, H, ctypes.byref(first)), E, "past n_cap"),
            (lambda: L.bk_collect_add_noised(engine.ctx, one, many, 65, 1, H, None), U,
             "BK_COLLECT_NOISE_MAX_K"),
            (lambda: L.bk_collect_add_noised(engine.ctx, null1, nzp, 2, 1, H, None), E, "null delta 0"),
            (lambda: L.bk_collect_add_noised(engine.ctx, two, None, 0, 2, H, None), E, "past n_cap"),
            (lambda: L.bk_collect_finish(engine.ctx, bad3.ctypes.data, 3, 1, sp, None, None, None), E,
             "no collected slot"),
            (lambda: L.bk_collect_finish(engine.ctx, None, n, 0, sp, None, None, None), E,
             "need 1 <= f < n"),
            (lambda: L.bk_collect_finish(engine.ctx, None, n, n, sp, None, None, None), E,
             "need 1 <= f < n"),
            (lambda: L.bk_collect_add_finish(engine.ctx, None, H, None, n + 1, f, None, sp, None, None,
                                             None), E, "null row 0"),
            (lambda: L.bk_collect_add_finish(engine.ctx, rp, H, rep3.ctypes.data, 3, 1, None, sp, None,
                                             None, None), E, "repeats a slot"),
            (lambda: L.bk_collect_add_finish(engine.ctx, rp, H, None, n + 1, n + 1, None, sp, None,
                                             None, None), E, "need 1 <= f < n"),
            (lambda: L.bk_collect_add_noised_finish(engine.ctx, rp, many, 65, H, None, n + 1, f, None,
                                                    sp, None, None, None), U, "BK_COLLECT_NOISE_MAX_K"),
            (lambda: L.bk_collect_add_noised_finish(engine.ctx, None, nzp, 2, H, None, n + 1, f, None,
                                                    sp, None, None, None), E, "null delta 0"),
            (lambda: L.bk_collect_add_noised_finish(engine.ctx, rp, nzp, 2, H, bad3.ctypes.data, 3, 1,
                                                    None, sp, None, None, None), E, "no collected slot"),
            (lambda: L.bk_collect_add_noised_finish(engine.ctx, rp, nzp, 2, H, None, n + 1, 0, None,
                                                    sp, None, None, None), E, "need 1 <= f < n"),
        ]
        for call, status, word in bad:
            assert call() == status, word
            assert word in _lib.last_error(), (word, _lib.last_error())
            assert engine.collect_count() == n and first.value == -7
        assert engine.collect_tiny_stats() == t0 and engine.collect_stats() == s0
        _assert_same(_finish(engine, f=f), ref, "after the refused calls")
        # past n_cap on the fused entries, once the collection is full
        assert engine.collect_add_ptr(src.ptrs(n, 1), 1, H) == n
        t0 = engine.collect_tiny_stats()
        assert L.bk_collect_add_finish(engine.ctx, rp, H, None, n + 2, f, None, sp, None, None,
                                       None) == E
        assert "past n_cap" in _lib.last_error()
        assert L.bk_collect_add_noised_finish(engine.ctx, rp, nzp, 2, H, None, n + 2, f, None, sp,
                                              None, None, None) == E
        assert "past n_cap" in _lib.last_error()
        assert engine.collect_count() == n + 1 and engine.collect_tiny_stats() == t0
        # an F32 collection refuses the noised forms
        engine.collect_begin(4, d, np.float32)
        assert L.bk_collect_add_noised(engine.ctx, one, nzp, 2, 1, H, None) == E
        assert "BK_F32" in _lib.last_error()
        assert L.bk_collect_add_noised_finish(engine.ctx, rp, nzp, 2, H, None, 1, 1, None, sp, None,
                                              None, None) == E
        assert "BK_F32" in _lib.last_error()
        assert engine.collect_count() == 0 and engine.collect_tiny_stats() == ZERO3
    finally:
        engine.set_collect_tiny(False)


def _creditcard_round(engine, oracle, tiny, noised):
    n, d = 10, 25
    X, _ = GU.build_input("A_creditcard", oracle)
    X = np.ascontiguousarray(X, dtype=np.float64)
    rng = np.random.default_rng(5)
    Nz = 1e-2 * rng.standard_normal((n, d))
    ids = [7 + 3 * i for i in range(n)]
    arrival = [int(i) for i in rng.permutation(n)]
    v = KRUMValidator(engine=engine, collect=True, noised=noised, tiny=tiny, n_cap=n).initialize()
    for q, i in enumerate(arrival):
        if noised:
            u = Update(SourceID=ids[i], Delta=X[i].copy(), Noise=Nz[i].copy())
        else:
            u = Update(SourceID=ids[i], NoisedDelta=X[i] + Nz[i])
        v.add_update(u, last=q == n - 1)
    return v


@pytest.mark.parametrize("noised", [False, True])
def test_krum_validator(engine, oracle, noised):
    try:
        ref = _creditcard_round(engine, oracle, False, noised)
        assert engine.collect_tiny_stats() == ZERO3
        got = _creditcard_round(engine, oracle, True, noised)
        assert engine.collect_tiny_stats() == {"adds": 9, "finishes": 0, "arrivals": 1}
        assert got.AcceptedList == ref.AcceptedList and len(got.AcceptedList) == 5
        assert [u.SourceID for u in got.UpdateList] == [u.SourceID for u in ref.UpdateList]
    finally:
        engine.set_collect_tiny(False)
