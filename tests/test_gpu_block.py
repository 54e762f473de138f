"""MI355X parity of the miner's block (bk_block_*) against the CPU oracle
(oracle/aggregate_oracle.c), bit for bit on view(np.int64): the running fp64
gradient against oracle.aggregate over the accepted slots in arrival order, the
running int64 sum and its quotient against oracle.qsum.

Every parity case first shows on the CPU that its rows can tell arrival orders
apart (the oracle's sum over the reversed order differs); seeds whose rows
cannot are skipped over by _case.

The mapped-arrival and mapped-output paths are taken up to measured sizes
(bk_ctx.h BLOCK_*_MAX): host rows up to d = 32,768 fp64 are read from the mapped
arrival block, a gradient up to d = 784 is stored into the mapped output, hence
the triples 783 / 784 / 785 and 32,767 / 32,768 / 32,769.  `cut_engine` is a
second engine whose three cuts the BK_BLOCK_* knobs put at 262,144 bytes, so
the mapped output also runs at sizes the product copies at.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

H, P, D = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
CUT_BYTES = 32768 * 8
N = 17
GROUPINGS = {"singly": [1] * 17, "3+8+6": [3, 8, 6], "17": [17], "9+8": [9, 8]}
MASKS = ["all", "none", "alternating", "last", "null"]


def _rand(n, d, seed, spread=True):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if spread:
        X *= 10.0 ** rng.integers(-6, 3, size=(n, 1))
    return X


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _mask(name, n=N):
    if name in ("all", "null"):
        return np.ones(n, dtype=np.uint8)
    if name == "none":
        return np.zeros(n, dtype=np.uint8)
    if name == "alternating":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    m = np.zeros(n, dtype=np.uint8)
    m[-1] = 1
    return m


_CASES = {}


def _case(oracle, n, d, dtype=np.float64):
    """(X, g0, {mask name: oracle gradient}) for n rows of d, computed once: the
    first seed whose rows tell the forward from the reversed order, for every
    mask with at least two accepted rows."""
    key = (n, d, np.dtype(dtype).name)
    if key in _CASES:
        return _CASES[key]
    for seed in range(1000 + d, 1064 + d):
        X = _rand(n, d, seed).astype(dtype)
        g0 = _rand(1, d, seed + 7)[0]
        X64 = X.astype(np.float64)
        want, ok = {}, True
        for name in MASKS:
            idx = np.flatnonzero(_mask(name, n)).astype(np.int64)
            want[name] = oracle.aggregate(X64, idx, g0)
            if len(idx) >= 2:
                rev = oracle.aggregate(X64, idx[::-1].copy(), g0)
                ok = ok and not np.array_equal(_bits(rev), _bits(want[name]))
        if ok:
            _CASES[key] = (X, g0, want)
            return _CASES[key]
    raise AssertionError("no seed of 64 tells arrival orders apart at n=%d d=%d" % (n, d))


class Rows:
    """Separately allocated rows at `where` (pinned rows are HIP's, 16-byte
    aligned; pageable rows start `off` bytes past a 16-byte boundary, device
    rows 8 bytes past one) and the pointer table the ABI takes."""

    def __init__(self, X, where, off=8):
        self.keep, ptrs = [], []
        es = X.dtype.itemsize
        tdt = torch.float64 if es == 8 else torch.float32
        for r in X:
            d = r.shape[0]
            pad = 16 // es
            if where == H:
                buf = np.empty(d + 2 * pad, dtype=X.dtype)
                o = (-buf.ctypes.data % 16 + off) // es
                row = buf[o:o + d]
                row[:] = r
                p = row.ctypes.data
                assert p % 16 == off % 16
            elif where == P:
                row = torch.from_numpy(np.ascontiguousarray(r)).pin_memory()
                buf, p = row, row.data_ptr()
            else:
                buf = torch.empty(d + 2 * pad, dtype=tdt, device="cuda")
                o = (-buf.data_ptr() % 16 + 8) // es
                row = buf[o:o + d]
                row.copy_(torch.from_numpy(np.ascontiguousarray(r)))
                p = row.data_ptr()
                assert p % 16 == 8
            self.keep.append(buf)
            ptrs.append(p)
        if where == D:
            torch.cuda.synchronize()
        self.ptrs = ptrs

    def table(self, lo, hi):
        return (ctypes.c_void_p * (hi - lo))(*self.ptrs[lo:hi])


def _add(engine, rows, lo, hi, where, mask):
    acc = None if mask is None else np.ascontiguousarray(mask[lo:hi])
    return engine.block_add_ptr(rows.table(lo, hi), hi - lo, where,
                                None if acc is None else acc.ctypes.data)


def _run(engine, X, g0, mask_name, grouping, where, prec=None, off=8, rows=None):
    rows = rows or Rows(X, where, off)
    mask = None if mask_name == "null" else _mask(mask_name, len(X))
    engine.block_begin(g0, prec, X.dtype)
    lo = 0
    for g in grouping:
        assert _add(engine, rows, lo, lo + g, where, mask) == lo
        lo += g
    assert lo == len(X)
    assert engine.block_count() == (len(X), int(_mask(mask_name, len(X)).sum()))
    return engine.block_finish(want_qsum=prec is not None)


@pytest.fixture(scope="module")
def cut_engine():
    """An engine whose block takes the mapped arrival block and the mapped
    output up to CUT_BYTES (the knobs of bk_create)."""
    from biscotti_amd.krum import Engine
    names = ("BK_BLOCK_MAPPED_HOST", "BK_BLOCK_MAPPED_PINNED", "BK_BLOCK_FIN")
    old = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ[k] = str(CUT_BYTES)
    try:
        e = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    e.close()


@pytest.fixture(params=["product", "cuts"])
def eng(request, engine):
    return engine if request.param == "product" else request.getfixturevalue("cut_engine")


PRECS = [None, 0, 4, 18]


@pytest.mark.parametrize("d", [1, 2, 3, 33, 783, 784, 785, 1001, 7850, 32767, 32768, 32769, 32770,
                               262147])
def test_parity_groupings_and_masks(eng, oracle, d):
    X, g0, want = _case(oracle, N, d)
    rows = Rows(X, H)
    qs = {}
    k = 0
    for mname in MASKS:
        idx = np.flatnonzero(_mask(mname)).astype(np.int64)
        for gname, grouping in GROUPINGS.items():
            prec = PRECS[k % 4]
            k += 1
            out = _run(eng, X, g0, mname, grouping, H, prec, rows=rows)
            g = out if prec is None else out[0]
            assert np.array_equal(_bits(g), _bits(want[mname])), (d, mname, gname)
            if prec is not None:
                if (mname, prec) not in qs:
                    qs[mname, prec] = oracle.qsum(X, idx, prec)
                ws, wf = qs[mname, prec]
                assert np.array_equal(out[1], ws), (d, mname, gname, prec)
                assert np.array_equal(_bits(out[2]), _bits(wf)), (d, mname, gname, prec)


@pytest.mark.parametrize("prec", [0, 4, 18])
@pytest.mark.parametrize("d", [33, 7850])
def test_parity_every_precision(eng, oracle, d, prec):
    X, g0, want = _case(oracle, N, d)
    g, s, sf = _run(eng, X, g0, "alternating", [3, 8, 6], H, prec)
    idx = np.flatnonzero(_mask("alternating")).astype(np.int64)
    ws, wf = oracle.qsum(X, idx, prec)
    assert np.array_equal(_bits(g), _bits(want["alternating"]))
    assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))


@pytest.mark.parametrize("where,off", [(H, 8), (P, 0), (D, 8)])
@pytest.mark.parametrize("d", [3, 1001, 32768, 32769])
def test_row_sources_f64(eng, oracle, d, where, off):
    X, g0, want = _case(oracle, N, d)
    g, s, sf = _run(eng, X, g0, "all", [9, 8], where, 4, off)
    ws, wf = oracle.qsum(X, np.arange(N, dtype=np.int64), 4)
    assert np.array_equal(_bits(g), _bits(want["all"]))
    assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))


@pytest.mark.parametrize("where,off", [(H, 4), (H, 8), (P, 0), (D, 8)])
@pytest.mark.parametrize("d", [4096, 4099])
def test_row_sources_f32(eng, oracle, d, where, off):
    X, g0, want = _case(oracle, N, d, np.float32)
    for mname, grouping in (("all", [3, 8, 6]), ("alternating", [1] * N)):
        g, s, sf = _run(eng, X, g0, mname, grouping, where, 4, off)
        idx = np.flatnonzero(_mask(mname)).astype(np.int64)
        ws, wf = oracle.qsum(X.astype(np.float64), idx, 4)
        assert np.array_equal(_bits(g), _bits(want[mname])), mname
        assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))


def _special(X, prec):
    """the values of test_gpu_aggregate._special, spread over arrivals 0, 1, 9,
    10 and 16: three launch groups when the rows arrive as 3 + 8 + 6"""
    X = X.copy()
    X[0, 0] = np.nan
    X[0, 1] = np.inf
    X[9, 1] = -np.inf
    X[1, 2] = -0.0
    X[10, 3] = 9.3e18 / 10.0 ** prec        # out of int64 range after scaling
    X[1, 4] = 9.2e18 / 10.0 ** prec         # in range; two of them wrap the sum
    X[16, 4] = 9.2e18 / 10.0 ** prec
    X[10, 5] = -1.99999 / 10.0 ** prec      # truncation toward zero -> -1
    return X


@pytest.mark.parametrize("prec", [0, 4, 18])
@pytest.mark.parametrize("d", [7, 1001])
def test_quantised_specials(eng, oracle, d, prec):
    X = _special(_rand(N, d, prec + d), prec)
    g0 = _rand(1, d, 5)[0]
    idx = np.arange(N, dtype=np.int64)
    ws, wf = oracle.qsum(X, idx, prec)
    # the gradient's own NaNs (inf - inf) carry the sign the adder gives them:
    # the contract there is bk_aggregate's bits, the same adds on the same GPU
    wg = eng.aggregate(X, idx, g0.copy())
    for grouping in ([3, 8, 6], [1] * N, [17]):
        g, s, sf = _run(eng, X, g0, "all", grouping, H, prec)
        assert np.array_equal(s, ws), grouping
        assert np.array_equal(_bits(sf), _bits(wf)), grouping
        assert np.array_equal(_bits(g), _bits(wg)), grouping
    fin = np.isfinite(wg)
    assert np.array_equal(_bits(wg[fin]), _bits(oracle.aggregate(X, idx, g0)[fin]))


@pytest.mark.parametrize("where", [H, P, D])
@pytest.mark.parametrize("acc_last", [1, 0])
@pytest.mark.parametrize("d", [33, 783, 784, 785, 32767, 32768, 32769])
def test_add_finish_is_add_then_finish(eng, oracle, d, acc_last, where):
    X, g0, _ = _case(oracle, N, d)
    rows = Rows(X, where)
    mask = _mask("all")
    mask[3] = 0
    mask[N - 3] = acc_last

    def two_calls():
        eng.block_begin(g0, 4)
        _add(eng, rows, 0, N - 3, where, mask)
        first = _add(eng, rows, N - 3, N - 2, where, mask)
        a = eng.block_finish(want_qsum=True)
        _add(eng, rows, N - 2, N, where, mask)
        return first, a, eng.block_finish(want_qsum=True), eng.block_count()

    first, a, b, cnt = two_calls()
    eng.block_begin(g0, 4)
    _add(eng, rows, 0, N - 3, where, mask)
    g = np.empty(d)
    s = np.empty(d, dtype=np.int64)
    sf = np.empty(d)
    st0 = eng.block_stats()
    slot = eng.block_add_finish_ptr(rows.ptrs[N - 3], acc_last, where, g.ctypes.data,
                                    s.ctypes.data, sf.ctypes.data)
    st1 = eng.block_stats()
    assert slot == first == N - 3
    assert np.array_equal(_bits(g), _bits(a[0]))
    assert np.array_equal(s, a[1]) and np.array_equal(_bits(sf), _bits(a[2]))
    _add(eng, rows, N - 2, N, where, mask)
    b2 = eng.block_finish(want_qsum=True)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(b, b2))
    assert eng.block_count() == cnt
    # the oracle on what both sequences hold in the end
    idx = np.flatnonzero(mask).astype(np.int64)
    assert np.array_equal(_bits(b2[0]), _bits(oracle.aggregate(X, idx, g0)))
    # the path taken: one fused launch up to the mapped-output cut, the two
    # calls' launches past it
    fused = _fin_at(eng, d)
    assert st1[1] - st0[1] == (1 if fused else 0)
    assert st1[0] - st0[0] == (0 if fused or not acc_last else 1)
    assert st1[3] - st0[3] == 1  # (the quotients always come through the mapped block)


def _fin_at(e, d):
    """whether the engine's gradient-only finish at d goes without a D2H copy
    (d doubles are within its mapped-output cut), read off its stats"""
    e.block_begin(np.zeros(d))
    e.block_finish()
    return e.block_stats()[3] == 1


def test_stats_show_the_path(cut_engine, oracle):
    # at the knob's cut: the rows through the mapped arrival block, the finish
    # through the mapped output
    X, g0, want = _case(oracle, N, 32768)
    for where in (H, P):
        rows = Rows(X, where)
        cut_engine.block_begin(g0)
        _add(cut_engine, rows, 0, N, where, None)
        assert cut_engine.block_stats() == [3, 0, 3, 0]
        g = cut_engine.block_finish()
        assert cut_engine.block_stats() == [3, 0, 3, 1]
        assert np.array_equal(_bits(g), _bits(want["all"]))
    # past it: copies both ways; device rows are never staged
    X2, g2, want2 = _case(oracle, N, 32770)
    for where in (H, P, D):
        rows = Rows(X2, where)
        cut_engine.block_begin(g2)
        _add(cut_engine, rows, 0, N, where, _mask("alternating"))
        g = cut_engine.block_finish()
        assert cut_engine.block_stats() == [3, 0, 0, 0]
        assert np.array_equal(_bits(g), _bits(want2["alternating"]))


def test_finish_does_not_consume_and_restart(eng, oracle):
    X, g0, want = _case(oracle, N, 1001)
    rows = Rows(X, H)
    eng.block_begin(g0, 4)
    _add(eng, rows, 0, N - 2, H, None)
    a = eng.block_finish(want_qsum=True)
    assert np.array_equal(_bits(a[0]), _bits(oracle.aggregate(X, np.arange(N - 2), g0)))
    assert np.array_equal(_bits(eng.block_finish()), _bits(a[0]))  # twice: the same
    _add(eng, rows, N - 2, N, H, None)
    g, s, sf = eng.block_finish(want_qsum=True)
    ws, wf = oracle.qsum(X, np.arange(N, dtype=np.int64), 4)
    assert np.array_equal(_bits(g), _bits(want["all"]))
    assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))
    # a smaller d, then a larger one: each starts from its own global_w
    for d in (33, 7850):
        Xd, gd, wd = _case(oracle, N, d)
        out = _run(eng, Xd, gd, "alternating", [9, 8], H, 0)
        assert np.array_equal(_bits(out[0]), _bits(wd["alternating"]))
        ws, _ = oracle.qsum(Xd, np.flatnonzero(_mask("alternating")).astype(np.int64), 0)
        assert np.array_equal(out[1], ws)
        assert eng.block_count() == (N, 9)


def _roni_round(engine, seed):
    """a logistic RONI round on the engine: set the validation set, begin, score"""
    rng = np.random.default_rng(seed)
    nv, d, n = 64, 25, 5
    Xv = np.ascontiguousarray(rng.standard_normal((nv, d)))
    yv = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
    ww = rng.standard_normal(d)
    deltas = np.ascontiguousarray(rng.standard_normal((n, d)) * 0.3)
    lib = _lib.lib()
    _lib.check(lib.bk_roni_set_validation(engine.ctx, Xv.ctypes.data, nv, d, d, yv.ctypes.data))
    _lib.check(lib.bk_roni_round_begin(engine.ctx, ww.ctypes.data, d, H))
    tab = (ctypes.c_void_p * n)(*[deltas[i].ctypes.data for i in range(n)])
    out = np.full(n, np.nan)
    _lib.check(lib.bk_roni_round_score(engine.ctx, tab, n, H, out.ctypes.data))
    return out


def _collection(engine, Y, between=None):
    engine.collect_begin(len(Y), Y.shape[1])
    for i, r in enumerate(Y):
        engine.collect_add(r)
        if between and i == len(Y) // 2:
            between()
    return engine.collect_finish(f=2)


def test_independent_of_other_calls(eng, oracle):
    X, g0, want = _case(oracle, N, 1001)
    rows = Rows(X, H)
    Y = _rand(12, 517, 3, spread=False)
    # the other calls on their own
    mk = eng.multikrum(Y, 3)
    col = _collection(eng, Y)
    roni = _roni_round(eng, 11)
    # the same calls between two adds of a block
    eng.block_begin(g0, 4)
    _add(eng, rows, 0, 9, H, None)
    mk2 = eng.multikrum(Y, 3)
    col2 = _collection(eng, Y)
    roni2 = _roni_round(eng, 11)
    _add(eng, rows, 9, N, H, None)
    g, s, sf = eng.block_finish(want_qsum=True)
    ws, wf = oracle.qsum(X, np.arange(N, dtype=np.int64), 4)
    assert np.array_equal(_bits(g), _bits(want["all"]))
    assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))
    for a, b in list(zip(mk, mk2)) + list(zip(col, col2)):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    assert np.array_equal(_bits(roni), _bits(roni2))
    # a block's adds between a collection's adds
    eng.block_begin(g0)

    def between():
        _add(eng, rows, 0, N, H, _mask("alternating"))
    col3 = _collection(eng, Y, between)
    for a, b in zip(col, col3):
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(eng.block_finish()), _bits(want["alternating"]))


def test_errors_leave_the_block_as_it_was(eng, oracle):
    X, g0, _ = _case(oracle, N, 33)
    rows = Rows(X, H)
    lib = _lib.lib()
    eng.block_begin(g0)  # (precision -1)
    _add(eng, rows, 0, 4, H, None)
    before = (eng.block_count(), eng.block_finish(), eng.block_stats()[:3])
    # a null row in the middle of a group of 9
    tab = rows.table(4, 13)
    tab[5] = None
    assert lib.bk_block_add(eng.ctx, tab, None, 9, H, None) == _lib.BK_EINVAL
    assert "rows[5]" in _lib.last_error()
    assert (eng.block_count(), eng.block_stats()[:3]) == (before[0], before[2])
    assert np.array_equal(_bits(eng.block_finish()), _bits(before[1]))
    # the quantised sum of a block that keeps none
    g = np.empty(33)
    s = np.empty(33, dtype=np.int64)
    sf = np.empty(33)
    assert lib.bk_block_finish(eng.ctx, g.ctypes.data, s.ctypes.data, None) == _lib.BK_EINVAL
    assert "precision" in _lib.last_error()
    assert lib.bk_block_finish(eng.ctx, g.ctypes.data, None, sf.ctypes.data) == _lib.BK_EINVAL
    assert lib.bk_block_add_finish(eng.ctx, rows.ptrs[4], 1, H, None, g.ctypes.data,
                                   s.ctypes.data, None) == _lib.BK_EINVAL
    assert (eng.block_count(), eng.block_stats()[:3]) == (before[0], before[2])
    assert np.array_equal(_bits(eng.block_finish()), _bits(before[1]))
    # more than BK_MAX_N rows in total (rejected ones count; none is read)
    many = (ctypes.c_void_p * _lib.BK_MAX_N)(*([rows.ptrs[0]] * _lib.BK_MAX_N))
    none = np.zeros(_lib.BK_MAX_N, dtype=np.uint8)
    assert lib.bk_block_add(eng.ctx, many, none.ctypes.data, _lib.BK_MAX_N, H,
                            None) == _lib.BK_EINVAL
    assert "BK_MAX_N" in _lib.last_error()
    assert eng.block_count() == before[0]
    # the block goes on
    _add(eng, rows, 4, N, H, None)
    assert np.array_equal(_bits(eng.block_finish()),
                          _bits(oracle.aggregate(X, np.arange(N, dtype=np.int64), g0)))


def test_calls_before_begin():
    """add, count, finish and stats on a context that never began a block"""
    from biscotti_amd.krum import Engine
    e = Engine(0)
    try:
        lib = _lib.lib()
        g = np.zeros(4)
        tab = (ctypes.c_void_p * 1)(g.ctypes.data)
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        out = (ctypes.c_int64 * 4)()
        for st in (lib.bk_block_add(e.ctx, tab, None, 1, H, None),
                   lib.bk_block_count(e.ctx, ctypes.byref(a), ctypes.byref(b)),
                   lib.bk_block_finish(e.ctx, g.ctypes.data, None, None),
                   lib.bk_block_add_finish(e.ctx, g.ctypes.data, 1, H, None, g.ctypes.data, None,
                                           None),
                   lib.bk_block_stats(e.ctx, out)):
            assert st == _lib.BK_EINVAL and "without bk_block_begin" in _lib.last_error()
    finally:
        e.close()


def test_large_pageable_rows_sampled_columns(engine, oracle):
    """64 rows x 1,048,579 fp64 (odd d), pageable, each through the pinned ring
    in 1 MiB pieces; checked on 4,096 sampled columns and the first and last 16."""
    n, d = 64, (1 << 20) + 3
    rng = np.random.default_rng(20)
    X = rng.standard_normal((n, d))
    X *= 10.0 ** rng.integers(-6, 3, size=(n, 1))
    g0 = rng.standard_normal(d)
    mask = np.ones(n, dtype=np.uint8)
    mask[[5, 40]] = 0
    cols = np.unique(np.concatenate([np.arange(16), np.arange(d - 16, d),
                                     rng.choice(d, 4096, replace=False)]))
    idx = np.flatnonzero(mask).astype(np.int64)
    Xs = np.ascontiguousarray(X[:, cols])
    want = oracle.aggregate(Xs, idx, g0[cols])
    rev = oracle.aggregate(Xs, idx[::-1].copy(), g0[cols])
    assert not np.array_equal(_bits(want), _bits(rev))
    ws, wf = oracle.qsum(Xs, idx, 4)
    engine.block_begin(g0, 4)
    lo = 0
    for g in [1] * 20 + [8, 11, 25]:
        tab = (ctypes.c_void_p * g)(*[X[i].ctypes.data for i in range(lo, lo + g)])
        engine.block_add_ptr(tab, g, H, mask[lo:lo + g].ctypes.data)
        lo += g
    assert engine.block_count() == (n, n - 2)
    g, s, sf = engine.block_finish(want_qsum=True)
    assert np.array_equal(_bits(g[cols]), _bits(want))
    assert np.array_equal(s[cols], ws) and np.array_equal(_bits(sf[cols]), _bits(wf))


@pytest.mark.parametrize("last,cut", [(True, None), (False, None), (True, 4)])
def test_block_collector_equals_create_block(eng, oracle, last, cut):
    from biscotti_amd.aggregate import PRECISION, STAKE_UNIT, BlockCollector, create_block
    from biscotti_amd.krum import Update
    d = 1003
    ups = [Update(SourceID=s, Delta=_rand(1, d, s)[0], Accepted=(s % 3 != 0))
           for s in (4, 1, 9, 6, 2, 8, 5)]
    ups = ups[:cut]  # the deadline path: fewer rows than expected
    g0 = _rand(1, d, 77)[0]
    stake_a, stake_b = {4: 100, 9: 50}, {4: 100, 9: 50}
    want = create_block(g0, ups, stake_a, engine=eng)
    bc = BlockCollector(g0, precision=PRECISION, engine=eng)
    for i, u in enumerate(ups):
        assert bc.add_update(u, last=last and i == len(ups) - 1) == i + 1
    got = bc.create_block(stake_b)
    assert np.array_equal(_bits(got), _bits(want))
    assert stake_a == stake_b and stake_b[4] == 100 + STAKE_UNIT
    acc = np.array([i for i, u in enumerate(ups) if u.Accepted], dtype=np.int64)
    ws, wf = oracle.qsum(np.stack([u.Delta for u in ups]), acc, PRECISION)
    s, sf = bc.quantized_sum()
    assert np.array_equal(s, ws) and np.array_equal(_bits(sf), _bits(wf))
    assert np.array_equal(_bits(got), _bits(oracle.aggregate(np.stack([u.Delta for u in ups]),
                                                             acc, g0)))
    bc.flush()
    assert np.array_equal(_bits(bc.create_block({})), _bits(g0))
