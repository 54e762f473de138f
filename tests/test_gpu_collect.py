"""Incremental Multi-Krum (bk_collect_*): each update is uploaded and folded
into a Gram kept by arrival slot when it arrives (VerifyUpdateKRUM's append,
DistSys/krum.go:291); the finish gathers the packed upper through the caller's
order and runs the unchanged K2 / K3 / K3b, and K4 on the row store.

The bar: the reference golden's selection; the selection and the mean BITWISE
those of bk_multikrum on the same rows in the finish's order (K4 adds the same
rows in the same order); the scores within 1e-9 of the packed call's largest
finite score (another summation order of the Gram) with the same NaN / inf
pattern; the same bits whatever the arrival order, the grouping of the adds
and the rows' memory, and from the same sequence of calls."""
import ctypes

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402
from biscotti_amd.krum import Engine, KRUMValidator, Update  # noqa: E402

_packed_cache = {}


def _case(name, engine, oracle):
    """(X, params, packed (sel, scores, mean), packed margin): computed once per
    case and shared, never modified"""
    if name not in _packed_cache:
        X, p = GU.build_input(name, oracle)
        X = np.ascontiguousarray(X)
        ref = engine.multikrum(X, p["f"])
        mg = engine.selection_margin()
        for a in (X,) + tuple(ref):
            a.setflags(write=False)
        _packed_cache[name] = (X, p, ref, mg)
    return _packed_cache[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_sel_mean(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[2]), _bits(ref[2]))


def _same(got, ref):
    return _same_sel_mean(got, ref) and np.array_equal(_bits(got[1]), _bits(ref[1]))


def _scores_close(sc, ref):
    """within 1e-9 of the reference's largest finite score, same NaN / inf pattern"""
    assert np.array_equal(np.isnan(sc), np.isnan(ref))
    assert np.array_equal(np.isposinf(sc), np.isposinf(ref))
    assert np.array_equal(np.isneginf(sc), np.isneginf(ref))
    fin = np.isfinite(ref)
    if fin.any():
        scale = np.max(np.abs(ref[fin]))
        err = np.max(np.abs(sc[fin] - ref[fin]))
        print("scores: max err %g, 1e-9 x scale %g" % (err, 1e-9 * scale))
        assert err <= 1e-9 * scale


def _collect_rows(engine, X, groups=None, n_cap=None):
    """begin, then add X's rows in order: one at a time, or in the given groups"""
    n, d = X.shape
    engine.collect_begin(n_cap or n, d, X.dtype)
    i = 0
    for g in groups or [1] * n:
        first = engine.collect_add([X[r] for r in range(i, i + g)])
        assert first == i
        i += g
    assert i == n and engine.collect_count() == n


@pytest.mark.parametrize("name", GU.small_cases())
def test_goldens_one_row_at_a_time(name, engine, oracle):
    X, p = GU.build_input(name, oracle)
    if p["error"]:
        _collect_rows(engine, np.ascontiguousarray(X))
        with pytest.raises(ValueError):
            engine.collect_finish(f=p["f"])
        return
    X, p, ref, ref_mg = _case(name, engine, oracle)
    _collect_rows(engine, X)
    got = engine.collect_finish(f=p["f"])
    mg = engine.selection_margin()
    g = GU.load(name)
    assert np.array_equal(got[0], g["sel"]), name
    GU.check_scores(got[1], g)
    GU.check_mean(got[2], g, GU.manifest()[name])
    assert _same_sel_mean(got, ref), name
    _scores_close(got[1], ref[1])
    assert (mg["d"], mg["k"], mg["near_tie"]) == (ref_mg["d"], ref_mg["k"], ref_mg["near_tie"])
    assert mg["d"] == p["d"]


@pytest.mark.parametrize("name", ["ragged_67x1003", "B_mnist"])
def test_arrival_order(name, engine, oracle):
    """rows arrive in a random order; the finish's order puts them back"""
    X, p, ref, _ = _case(name, engine, oracle)
    n = X.shape[0]
    perm = np.random.default_rng(7).permutation(n)  # slot s holds row perm[s]
    _collect_rows(engine, np.ascontiguousarray(X[perm]))
    order = np.empty(n, np.int64)
    order[perm] = np.arange(n)
    got = engine.collect_finish(order=order, f=p["f"])
    assert _same_sel_mean(got, ref)
    _scores_close(got[1], ref[1])


def test_subset_then_all_then_again(engine, oracle):
    name = "n129_d4097"
    X, p, ref, _ = _case(name, engine, oracle)
    _collect_rows(engine, X)
    subset = np.random.default_rng(11).choice(X.shape[0], size=70, replace=False).astype(np.int64)
    got = engine.collect_finish(order=subset, f=21)
    sub_ref = engine.multikrum(np.ascontiguousarray(X[subset]), 21)
    assert _same_sel_mean(got, sub_ref)
    _scores_close(got[1], sub_ref[1])
    # the finish did not consume the collection
    full = engine.collect_finish(f=p["f"])
    g = GU.load(name)
    assert np.array_equal(full[0], g["sel"])
    GU.check_scores(full[1], g)
    GU.check_mean(full[2], g, GU.manifest()[name])
    assert _same_sel_mean(full, ref)
    again = engine.collect_finish(f=p["f"])
    assert _same(again, full)


def test_batched_adds(engine, oracle):
    X, p, ref, _ = _case("ragged_67x1003", engine, oracle)
    groups = [1, 3, 16, 17, 30]
    assert sum(groups) == X.shape[0]
    _collect_rows(engine, X)
    single = engine.collect_finish(f=p["f"])
    _collect_rows(engine, X, groups)
    got = engine.collect_finish(f=p["f"])
    assert _same_sel_mean(got, ref)
    _scores_close(got[1], single[1])
    _collect_rows(engine, X, groups)
    rep = engine.collect_finish(f=p["f"])
    assert np.array_equal(_bits(rep[1]), _bits(got[1]))
    # every Gram element's summation order depends on (d, dtype) alone (bk.h)
    assert np.array_equal(_bits(got[1]), _bits(single[1]))


def test_row_sources(engine, oracle):
    """pageable rows off 16-B alignment, pinned rows and device rows"""
    X, p, ref, _ = _case("ragged_67x1003", engine, oracle)
    n, d = X.shape
    outs = []
    # pageable, each row at a 1-element offset of its own allocation
    keep = []
    for i in range(n):
        buf = np.empty(d + 1, dtype=X.dtype)
        buf[1:] = X[i]
        keep.append(buf[1:])
    assert any(a.ctypes.data % 16 for a in keep)
    engine.collect_begin(n, d, X.dtype)
    for a in keep:
        engine.collect_add(a)
    outs.append(engine.collect_finish(f=p["f"]))
    Xp = torch.from_numpy(np.array(X)).pin_memory()
    Xd = Xp.cuda()
    torch.cuda.synchronize()
    for t, where in ((Xp, _lib.BK_HOST_PINNED), (Xd, _lib.BK_DEVICE)):
        engine.collect_begin(n, d, X.dtype)
        for i in range(n):
            ptr = (ctypes.c_void_p * 1)(t.data_ptr() + i * d * X.itemsize)
            assert engine.collect_add_ptr(ptr, 1, where) == i
        outs.append(engine.collect_finish(f=p["f"]))
    assert _same(outs[1], outs[0]) and _same(outs[2], outs[0])
    assert _same_sel_mean(outs[0], ref)


def test_batch_calls_between_adds_leave_the_collection_intact(engine, oracle):
    X, p, ref, _ = _case("ragged_67x1003", engine, oracle)
    n, d = X.shape
    _collect_rows(engine, X)
    plain = engine.collect_finish(f=p["f"])
    Y = oracle.synth(300, 5000, 5, 90)   # the general path: K1 workspace, packed upper, K4
    Z = oracle.synth(10, 25, 6, 2)       # the one-launch path
    engine.collect_begin(n, d, X.dtype)
    for i in range(n):
        engine.collect_add(X[i])
        if i == 20:
            assert np.array_equal(engine.multikrum(Y, 90)[0], oracle.krum(Y, 90)[0])
        if i == 40:
            engine.multikrum(Z, 2)
    got = engine.collect_finish(f=p["f"])
    assert _same(got, plain)
    assert _same_sel_mean(got, ref)


def test_restart_discards_the_rows(engine, oracle):
    X, p, _, _ = _case("n129_d4097", engine, oracle)
    _collect_rows(engine, X)
    Y, q, yref, _ = _case("ragged_67x1003", engine, oracle)
    engine.collect_begin(Y.shape[0], Y.shape[1], Y.dtype)
    assert engine.collect_count() == 0
    for i in range(Y.shape[0]):
        engine.collect_add(Y[i])
    got = engine.collect_finish(f=q["f"])
    assert np.array_equal(got[0], GU.load("ragged_67x1003")["sel"])
    assert _same_sel_mean(got, yref)


def test_errors_leave_the_collection_usable(engine, oracle):
    X, p, ref, _ = _case("ragged_67x1003", engine, oracle)
    n, d = X.shape
    f = p["f"]
    L = _lib.lib()
    sel, mo = np.empty(n, np.int64), ctypes.c_int64(0)

    def finish_raw(ctx, order, nn, ff):
        return L.bk_collect_finish(ctx, order.ctypes.data if order is not None else None, nn, ff,
                                   sel.ctypes.data, ctypes.addressof(mo), None, None)

    # finish (and add) before begin, on a context that never began
    fresh = Engine(0)
    try:
        assert finish_raw(fresh.ctx, None, n, f) == _lib.BK_EINVAL
        assert "without bk_collect_begin" in _lib.last_error()
        one = (ctypes.c_void_p * 1)(X[0].ctypes.data)
        assert L.bk_collect_add(fresh.ctx, one, 1, _lib.BK_HOST, None) == _lib.BK_EINVAL
        fresh.collect_begin(2, d, X.dtype)
        fresh.collect_add([X[0], X[1]])
        assert fresh.collect_count() == 2
    finally:
        fresh.close()

    engine.collect_begin(n, d, X.dtype)
    for i in range(n - 3):
        engine.collect_add(X[i])
    # a NULL row inside a batch: nothing is added
    ptrs = (ctypes.c_void_p * 3)(X[n - 3].ctypes.data, None, X[n - 1].ctypes.data)
    assert L.bk_collect_add(engine.ctx, ptrs, 3, _lib.BK_HOST, None) == _lib.BK_EINVAL
    assert "null row 1" in _lib.last_error()
    assert L.bk_collect_add(engine.ctx, None, 3, _lib.BK_HOST, None) == _lib.BK_EINVAL
    assert engine.collect_count() == n - 3
    assert engine.collect_add([X[n - 3], X[n - 2], X[n - 1]]) == n - 3
    # past n_cap
    with pytest.raises(ValueError):
        engine.collect_add(X[0])
    assert "past n_cap" in _lib.last_error()
    assert engine.collect_count() == n
    # order: a repeated slot, slots out of range
    order = np.arange(n, dtype=np.int64)
    for pos, bad in ((5, 4), (0, n), (n - 1, -1)):
        o = order.copy()
        o[pos] = bad
        assert finish_raw(engine.ctx, o, n, f) == _lib.BK_EINVAL, (pos, bad)
    assert finish_raw(engine.ctx, None, n - 1, f) == _lib.BK_EINVAL  # NULL order: n = count
    assert L.bk_collect_finish(engine.ctx, None, n, f, None, ctypes.addressof(mo), None,
                               None) == _lib.BK_EINVAL
    # f = 0 (the reference's argpartition ValueError) and f = n
    for bad_f in (0, n):
        assert finish_raw(engine.ctx, None, n, bad_f) == _lib.BK_EINVAL
        with pytest.raises(ValueError):
            engine.collect_finish(f=bad_f)
    assert L.bk_collect_begin(engine.ctx, _lib.BK_F64, _lib.BK_MAX_N + 1, d) == _lib.BK_EINVAL
    assert L.bk_collect_begin(engine.ctx, 7, n, d) == _lib.BK_EINVAL
    # ... and the collection is what it was
    assert engine.collect_count() == n
    got = engine.collect_finish(f=f)
    assert np.array_equal(got[0], GU.load("ragged_67x1003")["sel"])
    assert _same_sel_mean(got, ref)


def test_krum_validator_collect_mode(engine, oracle):
    """updates arriving in shuffled SourceID order accept the peers the default
    validator accepts on the SourceID-sorted batch"""
    n, d = 40, 1500
    X = oracle.synth(n, d, 31, 12)
    ids = [100 + 3 * i for i in range(n)]  # row i belongs to peer ids[i]
    base = KRUMValidator(engine=engine).initialize()
    base.UpdateList = [Update(SourceID=ids[i], NoisedDelta=X[i]) for i in range(n)]
    base.compute_scores()
    want = {base.UpdateList[i].SourceID for i in base.AcceptedList}
    v = KRUMValidator(engine=engine, collect=True, n_cap=n).initialize()
    for i in np.random.default_rng(3).permutation(n):
        v.add_update(Update(SourceID=ids[i], NoisedDelta=X[i]))
    v.compute_scores()
    assert [u.SourceID for u in v.UpdateList] == ids
    assert {v.UpdateList[i].SourceID for i in v.AcceptedList} == want
    assert len(want) == n - int(0.5 * n)
    for pid in ids:
        assert v.check_if_accepted(pid) == (pid in want)
    # the next round starts a new collection
    v.flush_collected_updates()
    v.add_update(Update(SourceID=1, NoisedDelta=X[0]))
    assert engine.collect_count() == 1
