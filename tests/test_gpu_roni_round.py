"""MI355X parity of the RONI rounds (bk_roni_round_* / bk_roni_softmax_round_*):
the iteration's model held on the GPU with its evaluation done, each update
scored on its own (Peer.VerifyUpdateRONI, DistSys/main.go:191-233).

The contract is bitwise: every score and every near-tie count equals what ONE
bk_roni / bk_roni_softmax call on the same ww and rows returns -- and so the
reference's goldens and the C oracle (oracle/roni_oracle.c).  Checked over the
goldens, over the shapes at which the round kernels change path (partial waves
and workgroups, the one-chunk / many-chunk switch, full and ragged groups of
BK_RONI_ROUND_G), over values that sit on the decision, over the three `where`s,
and over a round's lifetime."""
import ctypes

import numpy as np
import pytest

import roni_util as RU
import rsm_util as RSM

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

COUNTS = (1, 7, 8, 9, 17)  # a lone update, a full group, a split, a ragged tail


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _L():
    from biscotti_amd import _lib
    return _lib


class Rows:
    """count separately allocated rows at `where`, each 8-byte aligned and NOT
    16-byte aligned; keeps the storage alive and hands out the pointer table."""

    def __init__(self, D, where):
        L = _L()
        self.keep, ptrs = [], []
        for r in np.atleast_2d(D):
            d = r.shape[0]
            if where == L.BK_HOST:
                buf = np.empty(d + 2, dtype=np.float64)
            elif where == L.BK_HOST_PINNED:
                buf = torch.empty(d + 2, dtype=torch.float64).pin_memory()
            else:
                buf = torch.empty(d + 2, dtype=torch.float64, device="cuda")
            base = buf.ctypes.data if where == L.BK_HOST else buf.data_ptr()
            o = 1 if base % 16 == 0 else 0
            row = buf[o:o + d]
            if where == L.BK_HOST:
                row[:] = r
                p = row.ctypes.data
            else:
                row.copy_(torch.from_numpy(np.ascontiguousarray(r)))
                p = row.data_ptr()
            assert p % 16 == 8
            self.keep.append(buf)
            ptrs.append(p)
        if where == L.BK_DEVICE:
            torch.cuda.synchronize()
        self.n = len(ptrs)
        self.table = (ctypes.c_void_p * self.n)(*ptrs)


def _ww_at(ww, where):
    """(keep-alive, pointer) of ww at `where`."""
    L = _L()
    if where == L.BK_HOST:
        a = np.ascontiguousarray(ww, dtype=np.float64)
        return a, a.ctypes.data
    t = torch.from_numpy(np.ascontiguousarray(ww, dtype=np.float64))
    t = t.pin_memory() if where == L.BK_HOST_PINNED else t.cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def _padded(X, pad):
    """X with a row stride of X.shape[1] + pad (the padding holds NaNs)."""
    buf = np.full((X.shape[0], X.shape[1] + pad), np.nan, dtype=X.dtype)
    buf[:, :X.shape[1]] = X
    return buf


# ---- logistic ---------------------------------------------------------------
def _set_validation(engine, Xv, yv, pad=0):
    L = _L()
    Xp = _padded(np.asarray(Xv, dtype=np.float64), pad)
    y = np.ascontiguousarray(yv, dtype=np.float64)
    L.check(L.lib().bk_roni_set_validation(engine.ctx, Xp.ctypes.data, Xv.shape[0], Xv.shape[1],
                                           Xp.shape[1], y.ctypes.data))


def _begin(engine, ww, where=0):
    L = _L()
    keep, p = _ww_at(ww, where)
    L.check(L.lib().bk_roni_round_begin(engine.ctx, p, len(ww), where))
    return keep


def _score(engine, D, where=0):
    L = _L()
    rows = Rows(D, where)
    out = np.full(rows.n, np.nan)
    L.check(L.lib().bk_roni_round_score(engine.ctx, rows.table, rows.n, where, out.ctypes.data))
    return out


def _batched(engine, ww, D):
    L = _L()
    ww = np.ascontiguousarray(ww, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    out = np.full(len(D), np.nan)
    L.check(L.lib().bk_roni(engine.ctx, ww.ctypes.data, D.ctypes.data, len(D), D.shape[1],
                            D.shape[1], out.ctypes.data))
    return out


@pytest.mark.parametrize("name", RU.names())
def test_round_logistic_goldens(engine, name):
    Xv, yv, ww, deltas, want = RU.load(name)
    _set_validation(engine, Xv, yv)
    ref = _batched(engine, ww, deltas)
    assert np.array_equal(_bits(ref), _bits(want))
    _begin(engine, ww)
    one = np.concatenate([_score(engine, deltas[i:i + 1]) for i in range(len(deltas))])
    assert np.array_equal(_bits(one), _bits(want)), (name, one, want)
    allr = _score(engine, deltas)
    assert np.array_equal(_bits(allr), _bits(want)), (name, allr, want)


def _logistic_case(nv, d, n, seed):
    rng = np.random.default_rng(seed)
    Xv = np.hstack([np.ones((nv, 1)), rng.standard_normal((nv, d - 1))]) if d > 1 else \
        np.ones((nv, 1))
    yv = np.where(rng.standard_normal(nv) > 0, 1.0, -1.0)
    ww = rng.standard_normal(d)
    D = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 1, size=(n, 1))
    return Xv, yv, ww, D


@pytest.mark.parametrize("nv", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("d", [1, 25, 32, 33, 130])
def test_round_logistic_edges(engine, oracle, nv, d):
    """Partial waves and workgroups (one workgroup is its own last one out), the
    one-chunk / many-chunk switch at d = 32, a row of several chunks; Xv with
    ld > d; every group size; rows and ww at each `where` in turn."""
    Xv, yv, ww, D = _logistic_case(nv, d, max(COUNTS), 1000 * nv + d)
    want = oracle.roni(Xv, yv, ww, D)
    _set_validation(engine, Xv, yv, pad=3)
    ref = _batched(engine, ww, D)
    assert np.array_equal(_bits(ref), _bits(want))
    where = (nv + d) % 3
    keep = _begin(engine, ww, where=(where + 1) % 3)
    for i, count in enumerate(COUNTS):
        got = _score(engine, D[:count], where=(where + i) % 3)
        assert np.array_equal(_bits(got), _bits(want[:count])), (count, got, want[:count])
    del keep


def test_round_logistic_two_workgroup_rounds(engine, oracle):
    """More workgroups than one: the counts of 40 workgroups meet in the last."""
    Xv, yv, ww, D = _logistic_case(10_001, 25, 9, 5)
    want = oracle.roni(Xv, yv, ww, D)
    _set_validation(engine, Xv, yv)
    _begin(engine, ww)
    assert np.array_equal(_bits(_score(engine, D)), _bits(want))
    assert np.array_equal(_bits(_score(engine, D[4:5])), _bits(want[4:5]))


def test_round_logistic_decision_values(engine, oracle):
    """Xv . w exactly 0 (sign 0 matches no +-1 label), a NaN in one delta (only
    that update's score moves), an inf weight."""
    nv, d, n = 300, 25, 6
    Xv, yv, ww, D = _logistic_case(nv, d, n, 11)
    Xv[:40] = 0.0                      # dot = +0: np.sign gives 0
    Xv[40:60, 1:] = 0.0
    ww[0] = 0.0
    D[:, 0] = 0.0                      # rows 40..59: 1 * (0 + 0) + 0 ... = 0
    clean = D.copy()
    D[2, 7] = np.nan
    D[4, 3] = np.inf
    want = oracle.roni(Xv, yv, ww, D)
    want_clean = oracle.roni(Xv, yv, ww, clean)
    _set_validation(engine, Xv, yv)
    ref = _batched(engine, ww, D)
    assert np.array_equal(_bits(ref), _bits(want))
    _begin(engine, ww)
    got = _score(engine, D)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    one = np.concatenate([_score(engine, D[i:i + 1]) for i in range(n)])
    assert np.array_equal(_bits(one), _bits(want))
    keep = [i for i in range(n) if i not in (2, 4)]
    assert np.array_equal(_bits(got[keep]), _bits(want_clean[keep]))
    assert np.all(np.isfinite(got[keep]))


# ---- softmax ----------------------------------------------------------------
def _softmax_case(nv, din, C, n, seed, nan=False, ties=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((nv, din)).astype(np.float32)
    if ties:
        X[: max(1, nv // 4)] = 0.0  # every logit = its bias: exact ties between equal biases
    W = rng.standard_normal((C, din)) * 0.05
    b = rng.standard_normal(C) * 0.1
    if ties:
        b[:] = 0.25
    y = np.argmax(X.astype(np.float64) @ W.T + b, 1).astype(np.int32)
    flip = rng.random(nv) < 0.2
    y[flip] = (y[flip] + 1) % C
    ww = np.concatenate([W.ravel(), b])
    D = rng.standard_normal((n, ww.size)) * 10.0 ** rng.integers(-4, 0, size=(n, 1))
    if ties:
        D[:, C * din:] = 0.0  # the biases stay equal
    if nan:
        D[0, min(3, ww.size - 1)] = np.nan
        D[-1, -1] = np.inf
    return X, y, ww, D


def _sm_set_validation(engine, X, y, C, pad=0):
    L = _L()
    Xp = _padded(np.asarray(X, dtype=np.float32), pad)
    yy = np.ascontiguousarray(y, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_set_validation(engine.ctx, Xp.ctypes.data, X.shape[0],
                                                   X.shape[1], Xp.shape[1], yy.ctypes.data, C))


def _sm_begin(engine, ww, where=0):
    L = _L()
    keep, p = _ww_at(ww, where)
    L.check(L.lib().bk_roni_softmax_round_begin(engine.ctx, p, where))
    return keep


def _sm_score(engine, D, where=0, near=True):
    L = _L()
    rows = Rows(D, where)
    out = np.full(rows.n, np.nan)
    nt = np.full(rows.n + 1, -7, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_round_score(engine.ctx, rows.table, rows.n, where,
                                                out.ctypes.data, nt.ctypes.data if near else None))
    return out, nt


def _sm_batched(engine, ww, D):
    L = _L()
    ww = np.ascontiguousarray(ww, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    out = np.full(len(D), np.nan)
    nt = np.full(len(D) + 1, -7, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax(engine.ctx, ww.ctypes.data, D.ctypes.data, len(D), D.shape[1],
                                    out.ctypes.data, nt.ctypes.data))
    return out, nt


def _sm_check(engine, D, ref, rnt, where=0):
    got, nt = _sm_score(engine, D, where)
    n = len(D)
    assert np.array_equal(_bits(got), _bits(ref[:n])), (n, got, ref[:n])
    assert np.array_equal(nt, rnt[:n + 1]), (n, nt, rnt[:n + 1])


def _whole_set_goldens():
    import json
    import os
    cases = json.load(open(os.path.join(RSM.HERE, "roni_softmax_cases.json")))
    return sorted(k for k, p in cases.items() if p["nb"] >= p["nv"])


@pytest.mark.parametrize("name", _whole_set_goldens())
def test_round_softmax_goldens(engine, oracle, name):
    c = RSM.load(name)
    assert c["full"]
    D = c["D"][:17]  # (a whole-set golden has 30 updates of 7,850: 17 cover every group shape)
    want, wnt = oracle.roni_softmax(c["X"], c["y"], c["C"], c["ww"], D, near_ties=True)
    _sm_set_validation(engine, c["X"], c["y"], c["C"])
    ref, rnt = _sm_batched(engine, c["ww"], D)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    assert np.array_equal(_bits(ref), _bits(_sm_batched(engine, c["ww"], c["D"])[0][:17]))
    _sm_begin(engine, c["ww"])
    for i in range(len(D)):
        got, nt = _sm_score(engine, D[i:i + 1])
        assert _bits(got)[0] == _bits(ref)[i] and nt[0] == rnt[0] and nt[1] == rnt[1 + i]
    _sm_check(engine, D, ref, rnt)


@pytest.mark.parametrize("nv", [1, 65])
@pytest.mark.parametrize("C", [2, 10, 16])
@pytest.mark.parametrize("din", [1, 63, 65])
def test_round_softmax_edges(engine, oracle, nv, C, din):
    """One feature, a ragged chunk, a chunk and a tail; 2, 10 and 16 classes; one
    sample and a ragged fifth workgroup; Xv with ld > d_in; every group size."""
    X, y, ww, D = _softmax_case(nv, din, C, max(COUNTS), 100 * nv + 10 * C + din)
    want, wnt = oracle.roni_softmax(X, y, C, ww, D, near_ties=True)
    _sm_set_validation(engine, X, y, C, pad=5)
    ref, rnt = _sm_batched(engine, ww, D)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    where = (nv + C + din) % 3
    keep = _sm_begin(engine, ww, where=(where + 2) % 3)
    for i, count in enumerate(COUNTS):
        _sm_check(engine, D[:count], ref, rnt, where=(where + i) % 3)
    del keep


@pytest.mark.parametrize("kw", [{"ties": True}, {"nan": True}])
def test_round_softmax_decision_values(engine, oracle, kw):
    """Equal maximal logits (the first index wins), NaN and inf weights (a NaN
    logit wins the argmax; only that update's score moves)."""
    X, y, ww, D = _softmax_case(200, 70, 5, 9, 23, **kw)
    want, wnt = oracle.roni_softmax(X, y, 5, ww, D, near_ties=True)
    _sm_set_validation(engine, X, y, 5)
    ref, rnt = _sm_batched(engine, ww, D)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    _sm_begin(engine, ww)
    _sm_check(engine, D, ref, rnt)
    for i in (0, 4, 8):
        _sm_check(engine, D[i:i + 1], ref[i:i + 1], rnt[[0, 1 + i]])
    if "nan" in kw:
        clean = D.copy()
        clean[0] = 0.0
        clean[-1] = 0.0
        wc, wcn = oracle.roni_softmax(X, y, 5, ww, clean, near_ties=True)
        got, nt = _sm_score(engine, D)
        assert np.array_equal(_bits(got[1:-1]), _bits(wc[1:-1]))
        assert np.array_equal(nt[:-1][np.r_[0, 2:9]], wcn[:-1][np.r_[0, 2:9]])
    got, nt = _sm_score(engine, D[:3], near=False)  # near_ties is nullable
    assert np.array_equal(_bits(got), _bits(ref[:3])) and np.all(nt == -7)


# ---- a round's lifetime -------------------------------------------------------
def test_round_lifetime(engine, oracle):
    L = _L()
    lib = L.lib()
    Xv, yv, ww, D = _logistic_case(500, 25, 9, 3)
    rows = Rows(D, L.BK_HOST)
    out = np.zeros(len(D))
    _set_validation(engine, Xv, yv)  # a new set: no round is live
    assert lib.bk_roni_round_score(engine.ctx, rows.table, rows.n, 0, out.ctypes.data) == L.BK_EINVAL
    _begin(engine, ww)
    a = _score(engine, D)
    assert np.array_equal(_bits(a), _bits(oracle.roni(Xv, yv, ww, D)))
    # refused calls leave the round as it was
    assert lib.bk_roni_round_score(engine.ctx, rows.table, 0, 0, out.ctypes.data) == L.BK_EINVAL
    assert lib.bk_roni_round_score(engine.ctx, None, 1, 0, out.ctypes.data) == L.BK_EINVAL
    assert lib.bk_roni_round_score(engine.ctx, rows.table, rows.n, 0, None) == L.BK_EINVAL
    assert lib.bk_roni_round_score(engine.ctx, rows.table, rows.n, 3, out.ctypes.data) == L.BK_EINVAL
    assert lib.bk_roni_round_score(engine.ctx, rows.table, 65535, 0, out.ctypes.data) == L.BK_ENOTSUP
    hole = (ctypes.c_void_p * 2)(rows.table[0], None)
    assert lib.bk_roni_round_score(engine.ctx, hole, 2, 0, out.ctypes.data) == L.BK_EINVAL
    assert lib.bk_roni_round_begin(engine.ctx, None, 25, 0) == L.BK_EINVAL
    wwp = np.ascontiguousarray(ww)
    assert lib.bk_roni_round_begin(engine.ctx, wwp.ctypes.data, 24, 0) == L.BK_EINVAL
    assert lib.bk_roni_round_begin(engine.ctx, wwp.ctypes.data, 25, 7) == L.BK_EINVAL
    assert np.array_equal(_bits(_score(engine, D)), _bits(a))  # the same bits twice
    # other work on the context between begin and score
    rng = np.random.default_rng(0)
    engine.multikrum(rng.standard_normal((12, 40)), 3)
    tX = torch.from_numpy(rng.standard_normal((10, 64))).cuda()
    sel = torch.empty(7, dtype=torch.int64, device="cuda")
    engine.multikrum_device_ptr(tX.data_ptr(), L.BK_F64, 10, 64, 64, 3, sel.data_ptr())
    engine.collect_begin(8, 30)
    engine.collect_add([rng.standard_normal(30) for _ in range(3)])
    assert np.array_equal(_bits(_batched(engine, ww * 2.0, D)),
                          _bits(oracle.roni(Xv, yv, ww * 2.0, D)))  # a batched call, too
    assert np.array_equal(_bits(_score(engine, D)), _bits(a))
    # a second begin with another model changes the base
    ww2 = ww + 0.5 * np.random.default_rng(9).standard_normal(25)
    _begin(engine, ww2)
    b = _score(engine, D)
    assert np.array_equal(_bits(b), _bits(oracle.roni(Xv, yv, ww2, D)))
    assert not np.array_equal(_bits(a), _bits(b))
    # set_validation invalidates the round
    _set_validation(engine, Xv[:100], yv[:100])
    assert lib.bk_roni_round_score(engine.ctx, rows.table, rows.n, 0, out.ctypes.data) == L.BK_EINVAL
    assert "round" in L.last_error()


def test_round_softmax_lifetime(engine, oracle):
    L = _L()
    lib = L.lib()
    X, y, ww, D = _softmax_case(130, 40, 4, 5, 77)
    rows = Rows(D, L.BK_HOST)
    out = np.zeros(len(D))
    _sm_set_validation(engine, X, y, 4)
    assert lib.bk_roni_softmax_round_score(engine.ctx, rows.table, rows.n, 0, out.ctypes.data,
                                           None) == L.BK_EINVAL
    _sm_begin(engine, ww)
    ref, rnt = _sm_batched(engine, ww, D)  # (a batched call in between)
    _sm_check(engine, D, ref, rnt)
    assert lib.bk_roni_softmax_round_score(engine.ctx, rows.table, 0, 0, out.ctypes.data,
                                           None) == L.BK_EINVAL
    assert lib.bk_roni_softmax_round_score(engine.ctx, rows.table, rows.n, 0, None,
                                           None) == L.BK_EINVAL
    assert lib.bk_roni_softmax_round_begin(engine.ctx, None, 0) == L.BK_EINVAL
    _sm_check(engine, D, ref, rnt)
    ww2 = ww * 0.5
    _sm_begin(engine, ww2)
    want, wnt = oracle.roni_softmax(X, y, 4, ww2, D, near_ties=True)
    _sm_check(engine, D, want, wnt)
    _sm_set_validation(engine, X[:50], y[:50], 4)
    assert lib.bk_roni_softmax_round_score(engine.ctx, rows.table, rows.n, 0, out.ctypes.data,
                                           None) == L.BK_EINVAL


def test_round_timing_ids(engine):
    """The score launches are timed under their own kernel ids."""
    Xv, yv, ww, D = _logistic_case(300, 25, 9, 8)
    _set_validation(engine, Xv, yv)
    engine.timing_select(["k_roni", "k_roni_round"])
    try:
        _begin(engine, ww)
        _score(engine, D)      # 9 rows: two groups
        _score(engine, D[:1])
        t = engine.timing_read()
    finally:
        engine.timing_select([])
    assert t["k_roni"]["count"] == 1 and t["k_roni_round"]["count"] == 3


# ---- Python -------------------------------------------------------------------
def test_validator_rounds(engine):
    from biscotti_amd.krum import Update
    from biscotti_amd.roni import RONIValidator
    Xv, yv, ww, deltas, want = RU.load("roni_credit_like")
    v = RONIValidator(Xv, yv, engine=engine)
    ups = [Update(SourceID=i, NoisedDelta=deltas[i]) for i in range(len(deltas))]
    plain, rounds, s_plain, s_round = [], [], [], []
    for u in ups:
        plain.append(v.verify_update(u, ww))
        s_plain.append(v.last_score)
    assert v.rounds_begun == 0
    for u in ups:
        rounds.append(v.verify_update(u, ww.copy(), round=True))  # equal, not identical
        s_round.append(v.last_score)
    assert rounds == plain and plain[:8] == [True] * 8 and plain[8:] == [False] * 4
    assert np.array_equal(_bits(s_round), _bits(s_plain)) and np.array_equal(_bits(s_round), _bits(want))
    assert v.rounds_begun == 1
    ww2 = ww * 1.5
    assert v.verify_update(ups[0], ww2, round=True) == v.verify_update(ups[0], ww2)
    assert v.verify_update(ups[1], ww2, round=True) == v.verify_update(ups[1], ww2)
    assert v.rounds_begun == 2
    assert np.array_equal(_bits(v.score_round(list(deltas))), _bits(v.scores(ww2, deltas)))
    assert RONIValidator(Xv, yv, engine=engine, priv_prob=0.1).verify_update(ups[-1], ww, round=True)
    with pytest.raises(ValueError):
        RONIValidator(Xv, yv, engine=engine).score_round([deltas[0]])  # no round
    with pytest.raises(ValueError):
        v.score_round([deltas[0][:-1]])


def test_softmax_validator_rounds(engine):
    from biscotti_amd.krum import Update
    from biscotti_amd.roni import SoftmaxRONIValidator
    X, y, ww, D = _softmax_case(400, 100, 10, 6, 31)
    D[4:] *= 1e3 / np.abs(D[4:]).max()  # poisoned: large updates
    v = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=None)
    ups = [Update(SourceID=i, NoisedDelta=D[i]) for i in range(len(D))]
    for u in ups:
        a = v.verify_update(u, ww)
        sa, na = v.last_score, v.last_near_ties.copy()
        b = v.verify_update(u, ww, round=True)
        assert a == b and _bits(sa) == _bits(v.last_score)
        assert np.array_equal(v.last_near_ties, na) and v.last_idx is None
    assert v.rounds_begun == 1
    sc = v.scores(ww, D)
    nt = v.last_near_ties.copy()
    assert np.array_equal(_bits(v.score_round(list(D))), _bits(sc))
    assert np.array_equal(v.last_near_ties, nt)
    vb = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=1)
    with pytest.raises(ValueError):
        vb.verify_update(ups[0], ww, round=True)
    with pytest.raises(ValueError):
        vb.begin_round(ww)
