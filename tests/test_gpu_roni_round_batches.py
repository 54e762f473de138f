"""MI355X parity of the softmax round's mini-batch scoring
(bk_roni_softmax_round_score_batches): the iteration's model held on the GPU,
each update scored on its own two last mini-batches -- client_obj.roni as the
reference runs it (ML/Pytorch/client_obj.py:100-112, getTrainErr's last batch,
client.py:136-144; 10 samples, DistSys/honest.go:47).

The contract is bitwise: every score and every near-tie pair equals what ONE
bk_roni_softmax_batches call on the same ww, rows and idx returns -- and so the
C oracle (oracle/roni_oracle.c) and, up to flagged near ties, the reference's
goldens.  Checked over the goldens with their recorded batches, over the shapes
at which k_roni_round_batch changes path (tiles of 16 samples, chunks of 128
features, 2..16 classes, full and ragged groups of BK_RONI_ROUND_G, indices in
the launch's arguments or staged), over decision values, the three `where`s, a
round's lifetime, a bad index, and the Python validator."""
import ctypes

import numpy as np
import pytest

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
    """Separately allocated rows at `where`, each 8-byte aligned and NOT 16-byte
    aligned; keeps the storage alive and hands out the pointer table."""

    def __init__(self, D, where):
        L = _L()
        self.keep, ptrs = [], []
        for r in np.atleast_2d(D):
            d = r.shape[0]
            if where == L.BK_HOST:
                buf = np.empty(d + 2, dtype=np.float64)
                base = buf.ctypes.data
            else:
                buf = torch.empty(d + 2, dtype=torch.float64,
                                  device="cuda" if where == L.BK_DEVICE else "cpu")
                buf = buf.pin_memory() if where == L.BK_HOST_PINNED else buf
                base = buf.data_ptr()
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


def _case(nv, din, C, n, seed, nan=False, ties=False):
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


def _draw(nv, n, nb, seed):
    """(n, 2, nb) indices drawn WITH replacement (repeats inside a batch); every
    third update scores both evaluations on the same batch."""
    idx = np.random.default_rng(seed).integers(0, nv, size=(n, 2, nb), dtype=np.int64)
    idx[::3, 1] = idx[::3, 0]
    return idx


def _set_validation(engine, X, y, C, pad=0):
    L = _L()
    Xp = np.full((X.shape[0], X.shape[1] + pad), np.nan, dtype=np.float32)
    Xp[:, :X.shape[1]] = X
    yy = np.ascontiguousarray(y, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_set_validation(engine.ctx, Xp.ctypes.data, X.shape[0],
                                                   X.shape[1], Xp.shape[1], yy.ctypes.data, C))


def _begin(engine, ww):
    L = _L()
    w = np.ascontiguousarray(ww, dtype=np.float64)
    L.check(L.lib().bk_roni_softmax_round_begin(engine.ctx, w.ctypes.data, L.BK_HOST))


def _score(engine, D, idx, where=0, near=True):
    L = _L()
    rows = Rows(D, where)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    assert idx.shape[:2] == (rows.n, 2)
    out = np.full(rows.n, np.nan)
    nt = np.full((rows.n, 2), -7, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_round_score_batches(
        engine.ctx, rows.table, rows.n, where, idx.ctypes.data, idx.shape[2], out.ctypes.data,
        nt.ctypes.data if near else None))
    return out, nt


def _batched(engine, ww, D, idx):
    """ONE bk_roni_softmax_batches call: the contract's other side."""
    L = _L()
    ww = np.ascontiguousarray(ww, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = np.full(len(D), np.nan)
    nt = np.full((len(D), 2), -7, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_batches(engine.ctx, ww.ctypes.data, D.ctypes.data, len(D),
                                            D.shape[1], idx.ctypes.data, idx.shape[2],
                                            out.ctypes.data, nt.ctypes.data))
    return out, nt


def _whole(engine, D):
    L = _L()
    rows = Rows(D, L.BK_HOST)
    out = np.full(rows.n, np.nan)
    nt = np.full(rows.n + 1, -7, dtype=np.int32)
    L.check(L.lib().bk_roni_softmax_round_score(engine.ctx, rows.table, rows.n, L.BK_HOST,
                                                out.ctypes.data, nt.ctypes.data))
    return out, nt


def _check(engine, D, idx, ref, rnt, where=0):
    got, nt = _score(engine, D, idx, where)
    assert np.array_equal(_bits(got), _bits(ref)), (len(D), got, ref)
    assert np.array_equal(nt, rnt), (len(D), nt, rnt)


@pytest.mark.parametrize("name", RSM.names())
def test_round_batches_reference_goldens(engine, oracle, name):
    """Every golden with its recorded batches (nb = 3 .. 2,000): one update per
    call, as the verifier calls, and all updates in one call."""
    c = RSM.load(name)
    D, idx = c["D"], c["idx"]
    want, wnt = oracle.roni_softmax_batches(c["X"], c["y"], c["C"], c["ww"], D, idx)
    _set_validation(engine, c["X"], c["y"], c["C"])
    ref, rnt = _batched(engine, c["ww"], D, idx)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    _begin(engine, c["ww"])
    one = [_score(engine, D[i:i + 1], idx[i:i + 1]) for i in range(len(D))]
    assert np.array_equal(_bits(np.concatenate([o[0] for o in one])), _bits(want))
    assert np.array_equal(np.concatenate([o[1] for o in one]), wnt)
    _check(engine, D, idx, want, wnt)
    RSM.agree(ref, rnt, c["scores"], c["nb"])  # == the reference, or flagged


@pytest.mark.parametrize("nv,din,C,nb", [
    (50, 1, 2, 1),        # one feature, one sample
    (50, 63, 10, 10),     # Biscotti's batch; a ragged chunk
    (50, 64, 16, 15),     # every thread a logit; four whole float4 groups
    (50, 65, 2, 16),      # a full tile; a one-feature tail
    (50, 127, 10, 17),    # two tiles, the second of one sample; a chunk short of one feature
    (50, 128, 16, 37),    # three tiles; exactly one chunk
    (50, 129, 10, 10),    # a chunk and one feature
    (50, 300, 16, 37),    # three chunks, three tiles, 16 classes
    (1, 64, 10, 10),      # one validation sample: every index the same
    (1, 300, 2, 17),
])
def test_round_batches_edges(engine, oracle, nv, din, C, nb):
    """Xv with ld > d_in; every group size (counts 1 and 7 at nb <= 16 carry
    their indices in the launch's arguments, the larger ones stage them);
    repeated indices; rows at each `where` in turn."""
    n = max(COUNTS)
    X, y, ww, D = _case(nv, din, C, n, 1000 * nv + 10 * din + C + nb)
    idx = _draw(nv, n, nb, nv + din + nb)
    want, wnt = oracle.roni_softmax_batches(X, y, C, ww, D, idx)
    _set_validation(engine, X, y, C, pad=5)
    ref, rnt = _batched(engine, ww, D, idx)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    _begin(engine, ww)
    where = (nv + din + C + nb) % 3
    for i, count in enumerate(COUNTS):
        _check(engine, D[:count], idx[:count], want[:count], wnt[:count], where=(where + i) % 3)
    # a lone update that is not the first: its own rows of idx
    _check(engine, D[11:12], idx[11:12], want[11:12], wnt[11:12])


@pytest.mark.parametrize("kw", [{"ties": True}, {"nan": True}])
def test_round_batches_decision_values(engine, oracle, kw):
    """Equal maximal logits (the first index wins), NaN and inf weights (a NaN
    logit wins the argmax; only that update's score moves)."""
    X, y, ww, D = _case(200, 70, 5, 9, 23, **kw)
    idx = _draw(200, 9, 16, 5)
    if "ties" in kw:
        idx[:, :, :8] = np.arange(8)  # the zero samples: exact ties
    want, wnt = oracle.roni_softmax_batches(X, y, 5, ww, D, idx)
    _set_validation(engine, X, y, 5)
    ref, rnt = _batched(engine, ww, D, idx)
    assert np.array_equal(_bits(ref), _bits(want)) and np.array_equal(rnt, wnt)
    _begin(engine, ww)
    _check(engine, D, idx, want, wnt)
    for i in (0, 4, 8):
        _check(engine, D[i:i + 1], idx[i:i + 1], want[i:i + 1], wnt[i:i + 1])
    got, nt = _score(engine, D[:3], idx[:3], near=False)  # near_ties is nullable
    assert np.array_equal(_bits(got), _bits(want[:3])) and np.all(nt == -7)


def test_round_batches_where(engine, oracle):
    """Pageable rows off 16-byte alignment, pinned rows and device rows: the same bits."""
    L = _L()
    X, y, ww, D = _case(300, 200, 10, 9, 41)
    idx = _draw(300, 9, 10, 42)
    want, wnt = oracle.roni_softmax_batches(X, y, 10, ww, D, idx)
    _set_validation(engine, X, y, 10)
    _begin(engine, ww)
    for where in (L.BK_HOST, L.BK_HOST_PINNED, L.BK_DEVICE):
        _check(engine, D, idx, want, wnt, where=where)
        _check(engine, D[5:6], idx[5:6], want[5:6], wnt[5:6], where=where)


def test_round_batches_lifetime(engine, oracle):
    L = _L()
    lib = L.lib()
    X, y, ww, D = _case(130, 40, 4, 9, 77)
    idx = _draw(130, 9, 10, 78)
    rows = Rows(D, L.BK_HOST)
    out = np.zeros(len(D))

    def raw(table=rows.table, count=rows.n, where=0, ix=idx, nb=10, sc=out):
        return lib.bk_roni_softmax_round_score_batches(
            engine.ctx, table, count, where, ix.ctypes.data if ix is not None else None, nb,
            sc.ctypes.data if sc is not None else None, None)

    _set_validation(engine, X, y, 4)  # a new set: no round is live
    assert raw() == L.BK_EINVAL and "round" in L.last_error()
    _begin(engine, ww)
    want, wnt = oracle.roni_softmax_batches(X, y, 4, ww, D, idx)
    _check(engine, D, idx, want, wnt)
    # refused calls leave the round as it was
    assert raw(table=None) == L.BK_EINVAL
    assert raw(ix=None) == L.BK_EINVAL
    assert raw(sc=None) == L.BK_EINVAL
    assert raw(count=0) == L.BK_EINVAL
    assert raw(nb=0) == L.BK_EINVAL
    assert raw(where=3) == L.BK_EINVAL
    big = np.zeros(2 * 262140, dtype=np.int64)  # checked before the rows and the indices
    assert raw(count=262140, ix=big, nb=1) == L.BK_ENOTSUP
    hole = (ctypes.c_void_p * 2)(rows.table[0], None)
    assert raw(table=hole, count=2) == L.BK_EINVAL and "deltas[1]" in L.last_error()
    _check(engine, D, idx, want, wnt)
    # whole-set and mini-batch scores interleaved on one round
    wref, wrnt = _whole(engine, D)
    full, fnt = oracle.roni_softmax(X, y, 4, ww, D, near_ties=True)
    assert np.array_equal(_bits(wref), _bits(full)) and np.array_equal(wrnt, fnt)
    _check(engine, D[:1], idx[:1], want[:1], wnt[:1])
    w2, n2 = _whole(engine, D[3:4])
    assert _bits(w2)[0] == _bits(full)[3] and n2.tolist() == [fnt[0], fnt[4]]
    _check(engine, D, idx, want, wnt)
    # other work on the context between two scores
    rng = np.random.default_rng(0)
    b, bnt = _batched(engine, ww * 2.0, D, idx)
    w2x, w2n = oracle.roni_softmax_batches(X, y, 4, ww * 2.0, D, idx)
    assert np.array_equal(_bits(b), _bits(w2x)) and np.array_equal(bnt, w2n)
    engine.multikrum(rng.standard_normal((12, 40)), 3)
    engine.collect_begin(8, 30)
    engine.collect_add([rng.standard_normal(30) for _ in range(3)])
    _check(engine, D, idx, want, wnt)
    # a second begin with another model
    _begin(engine, ww * 0.5)
    want2, wnt2 = oracle.roni_softmax_batches(X, y, 4, ww * 0.5, D, idx)
    _check(engine, D, idx, want2, wnt2)
    # set_validation ends the round
    _set_validation(engine, X[:50], y[:50], 4)
    assert raw() == L.BK_EINVAL and "round" in L.last_error()


def test_round_batches_bad_index(engine, oracle):
    """An index outside [0, nv) is refused on the host with the update and the
    position named; the next valid score is what it would have been."""
    L = _L()
    X, y, ww, D = _case(100, 20, 4, 9, 1)
    idx = _draw(100, 9, 5, 2)
    want, wnt = oracle.roni_softmax_batches(X, y, 4, ww, D, idx)
    _set_validation(engine, X, y, 4)
    _begin(engine, ww)
    _check(engine, D[:2], idx[:2], want[:2], wnt[:2])
    for (j, e, s, v) in ((7, 1, 2, 100), (0, 0, 0, -1), (8, 0, 4, 1 << 40)):
        bad = idx.copy()
        bad[j, e, s] = v
        with pytest.raises(ValueError) as ei:
            _score(engine, D, bad)
        msg = str(ei.value)
        assert "update %d" % j in msg and "evaluation %d" % e in msg and "position %d" % s in msg, msg
        _check(engine, D, idx, want, wnt)


def test_round_batches_validator(engine, oracle):
    from biscotti_amd.krum import Update
    from biscotti_amd.roni import SoftmaxRONIValidator
    X, y, ww, D = _case(400, 100, 10, 6, 31)
    D[4:] *= 1e3 / np.abs(D[4:]).max()  # poisoned: large updates
    ups = [Update(SourceID=i, NoisedDelta=D[i]) for i in range(len(D))]
    plain = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=5)
    verdicts, scores, idxs = [], [], []
    for u in ups:
        verdicts.append(plain.verify_update(u, ww))
        scores.append(plain.last_score)
        idxs.append(plain.last_idx[0])
    v = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=5, round_batches=True)
    got, gs = [], []
    for u in ups:
        got.append(v.verify_update(u, ww.copy(), round=True))  # equal, not identical
        gs.append(v.last_score)
        assert v.last_idx.shape == (1, 2, 10) and v.last_near_ties.shape == (1, 2)
        assert np.array_equal(v.last_idx[0], idxs[len(got) - 1])
    assert got == verdicts and np.array_equal(_bits(gs), _bits(scores))
    assert v.rounds_begun == 1
    v.verify_update(ups[0], ww * 1.5, round=True)
    v.verify_update(ups[1], ww * 1.5, round=True)
    assert v.rounds_begun == 2
    # a fixed seed reproduces scores() of a same-seed validator; last_idx reproduces a call
    a = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=9)
    b = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=9, round_batches=True)
    sa = a.scores(ww, D)
    b.begin_round(ww)
    sb = b.score_round(list(D))
    assert np.array_equal(_bits(sa), _bits(sb))
    assert np.array_equal(a.last_idx, b.last_idx) and b.last_idx.shape == (6, 2, 10)
    assert np.array_equal(a.last_near_ties, b.last_near_ties) and b.last_near_ties.shape == (6, 2)
    want, wnt = oracle.roni_softmax_batches(X, y, 10, ww, D, b.last_idx)
    assert np.array_equal(_bits(sb), _bits(want)) and np.array_equal(b.last_near_ties, wnt)
    again = b.score_round(list(D), idx=b.last_idx)
    assert np.array_equal(_bits(again), _bits(sb))
    # the default validator still has no mini-batch rounds
    d = SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10, seed=1)
    with pytest.raises(ValueError):
        d.verify_update(ups[0], ww, round=True)
    with pytest.raises(ValueError):
        d.begin_round(ww)
    with pytest.raises(ValueError):
        SoftmaxRONIValidator(X, y, 10, engine=engine, batch_size=10,
                             round_batches=True).score_round([D[0]])  # no round
