"""MI355X: the miner's G1 point sums (bk_commit_points_*) against tests/commit_ref.py,
all 64 bytes of every output point, folded slot by slot as aggregateSecret folds.
Points are drawn per (slot, point number) from a pool of random multiples of G,
their negations and infinity.  NP is 3, 19 and 259 (past a workgroup at one lane)."""
import functools
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import commit_ref as C  # noqa: E402
from biscotti_amd import _lib, commit  # noqa: E402

H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
SHAPES = [(1, 1), (3, 5), (43, 5)]
SLOTS = 33


@functools.lru_cache(maxsize=None)
def _pool():
    rng = random.Random(28)
    pts = [C.mul(C.G, rng.randrange(1, C.N)) for _ in range(31)]
    pts = pts + [C.neg(a) for a in pts] + [C.INF, C.INF]
    return pts, [C.marshal(a) for a in pts]


@functools.lru_cache(maxsize=None)
def _parts(chunks, held):
    """SLOTS + 1 parts of pool indices, one per point number."""
    rng = random.Random(1000 * chunks + held)
    np_ = 1 + chunks * (1 + held)
    return [[rng.randrange(64) for _ in range(np_)] for _ in range(SLOTS + 1)]


def _split(row, chunks, held):
    """A row of 64-byte strings in the store's order -> the three arrays."""
    com = np.frombuffer(row[0], dtype=np.uint8).copy()
    per = [row[1 + c * (1 + held):1 + (c + 1) * (1 + held)] for c in range(chunks)]
    chk = C.as_array([p[0] for p in per])
    wit = C.as_array([w for p in per for w in p[1:]]).reshape(chunks, held, 64)
    return com, chk, wit


def _fold(rows):
    """The oracle's sum of rows of points, as the three arrays' bytes in row order."""
    acc = list(rows[0])
    for r in rows[1:]:
        acc = [C.add(a, b) for a, b in zip(acc, r)]
    return [C.marshal(a) for a in acc]


@functools.lru_cache(maxsize=None)
def _want(chunks, held, slots):
    pts = _pool()[0]
    parts = _parts(chunks, held)
    return _fold([[pts[i] for i in parts[s]] for s in slots])


@functools.lru_cache(maxsize=None)
def _list(n):
    return tuple(random.Random(n).sample(range(SLOTS), n))


_held = [None]


def _store(engine, chunks, held):
    """Make the (chunks, held) store of SLOTS parts the engine's (once per change)."""
    if _held[0] != (chunks, held):
        _held[0] = None
        raw = _pool()[1]
        engine.commit_points_begin(chunks, held, SLOTS + 1)
        for s in range(SLOTS):
            assert engine.commit_points_add(*_split([raw[i] for i in _parts(chunks, held)[s]],
                                                    chunks, held)) == s
        _held[0] = (chunks, held)
    return 1 + chunks * (1 + held)


def _got(outs):
    com, chk, wit = outs
    return [com.tobytes()] + [b for c in range(chk.shape[0])
                              for b in [chk[c].tobytes()] + [w.tobytes() for w in wit[c]]]


@pytest.mark.parametrize("lanes", [0, 1, 2, 8, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 33])
@pytest.mark.parametrize("shape", SHAPES)
def test_sum_shapes_lists_and_lanes(engine, shape, n, lanes):
    np_ = _store(engine, *shape)
    engine.commit_points_set_lanes(lanes)
    try:
        before = engine.commit_points_stats()
        got = _got(engine.commit_points_sum(np.array(_list(n))))
        after = engine.commit_points_stats()
    finally:
        engine.commit_points_set_lanes(0)
    assert got == _want(*shape, _list(n))
    assert [a - b for a, b in zip(after, before)] == [1, 4, 1, 0] and after[3] == SLOTS * np_
    if lanes == 0 and n > 1:  # the list's order changes no byte
        assert _got(engine.commit_points_sum(np.array(_list(n)[::-1]))) == got


class Buf:
    """Bytes at `where` between two 64-byte guard bands; host() reads all of it back."""

    def __init__(self, a, where):
        a = np.concatenate([np.full(64, 0xAB, np.uint8), np.ascontiguousarray(a).reshape(-1),
                            np.full(64, 0xAB, np.uint8)])
        self.where, self.t = where, a
        if where != H:
            self.t = torch.from_numpy(a).pin_memory() if where == PIN else torch.from_numpy(a).cuda()
            torch.cuda.synchronize()
        self.ptr = (a.ctypes.data if where == H else self.t.data_ptr()) + 64

    def host(self):
        a = self.t if self.where == H else self.t.cpu().numpy()
        assert (a[:64] == 0xAB).all() and (a[-64:] == 0xAB).all()
        return a[64:-64].tobytes()


@pytest.mark.parametrize("where", [H, PIN, DEV])
def test_placement_and_each_output_alone(engine, where):
    chunks, held = 3, 5
    _held[0] = None
    raw = _pool()[1]
    engine.commit_points_begin(chunks, held, 17)
    for s in range(17):
        bufs = [Buf(a, where) for a in _split([raw[i] for i in _parts(chunks, held)[s]], chunks, held)]
        assert engine.commit_points_add_ptr(*[b.ptr for b in bufs], where) == s
    assert engine.commit_points_count() == 17
    slots = np.arange(17, dtype=np.int64)[::-1].copy()
    want = b"".join(_want(chunks, held, tuple(range(17))))
    sizes = (64, chunks * 64, chunks * held * 64)
    for keep in ((0, 1, 2), (0,), (1,), (2,)):
        outs = [Buf(np.full(n, 0xCD, np.uint8), where) if i in keep else None
                for i, n in enumerate(sizes)]
        engine.commit_points_sum_ptr(slots, where, *[o.ptr if o else None for o in outs])
        com, chk, wit = [o.host() if o else None for o in outs]
        rows = _got((np.frombuffer(com or bytes(64), np.uint8),
                     np.frombuffer(chk or bytes(sizes[1]), np.uint8).reshape(chunks, 64),
                     np.frombuffer(wit or bytes(sizes[2]), np.uint8).reshape(chunks, held, 64)))
        for k, (g, w) in enumerate(zip(rows, [want[i:i + 64] for i in range(0, len(want), 64)])):
            which = 0 if k == 0 else (1 if (k - 1) % (1 + held) == 0 else 2)
            assert g == (w if which in keep else bytes(64)), (keep, k)


def test_crafted_store_doubling_and_infinity(engine):
    """Point 1 the same in every slot (doubling in the gather and in the tree),
    point 2 pairs P, -P, P', -P' (sums pass through infinity), point 3 infinity
    in every slot; then a 1 x 1 store whose every result is infinity."""
    pts, raw = _pool()
    _held[0] = None
    rows = [list(_parts(3, 5)[s]) for s in range(4)]
    for s, r in enumerate(rows):
        r[1], r[2], r[3] = 5, (7, 7 + 31, 9, 9 + 31)[s], 62
    store = commit.PointStore(3, 5, 4, engine=engine)
    for s, r in enumerate(rows):
        store.add_part("node%d" % s, *_split([raw[i] for i in r], 3, 5))
    want = _fold([[pts[i] for i in r] for r in rows])
    assert want[1] == C.marshal(C.mul(pts[5], 4)) and want[2] == want[3] == C.ZERO64
    for lanes in (0, 1, 2, 4, 8, 16):
        engine.commit_points_set_lanes(lanes)
        for order in (["node0", "node1", "node2", "node3"], ["node2", "node0", "node3", "node1"]):
            assert _got(store.miner_points(order)) == want, (lanes, order)
    zero = commit.PointStore(1, 1, 2, engine=engine)
    zero.add_part(0, *_split([raw[3], raw[3 + 31], raw[62]], 1, 1))
    zero.add_part(1, *_split([raw[3 + 31], raw[3], raw[63]], 1, 1))
    for lanes in (1, 2, 0):
        engine.commit_points_set_lanes(lanes)
        assert _got(zero.miner_points([1, 0])) == [C.ZERO64] * 3


def test_store_is_not_consumed(engine):
    shape = (3, 5)
    _store(engine, *shape)
    sub = _list(17)[:9]
    first = _got(engine.commit_points_sum(np.array(sub)))
    assert first == _want(*shape, sub)
    assert _got(engine.commit_points_sum(np.array(sorted(sub)))) == first
    raw = _pool()[1]
    _held[0] = None
    assert engine.commit_points_add(*_split([raw[i] for i in _parts(*shape)[SLOTS]], *shape)) == SLOTS
    assert _got(engine.commit_points_sum(np.array(sub))) == first
    assert _got(engine.commit_points_sum(np.array(sub + (SLOTS,)))) == _want(*shape, sub + (SLOTS,))
    with pytest.raises(ValueError, match="listed twice"):
        engine.commit_points_sum(np.array([3, 4, 3]))
    with pytest.raises(ValueError, match=r"slots\[1\]=34"):
        engine.commit_points_sum(np.array([3, 34]))


@pytest.mark.parametrize("k", [1 + 6, 1 + 6 + 3], ids=["chunk", "witness"])
@pytest.mark.parametrize("kind", ["x=p", "y+1"])
def test_invalid_part_takes_no_slot(engine, kind, k):
    chunks, held = 3, 5
    pts, raw = _pool()
    _held[0] = None
    engine.commit_points_begin(chunks, held, 4)
    good = [raw[i] for i in _parts(chunks, held)[0]]
    assert engine.commit_points_add(*_split(good, chunks, held)) == 0
    x, y = C.affine(pts[0])
    bad = list(good)
    bad[k] = (C.P.to_bytes(32, "big") + bad[k][32:]) if kind == "x=p" else \
        (x.to_bytes(32, "big") + ((y + 1) % C.P).to_bytes(32, "big"))
    bad[k + 4] = bad[k]  # the smallest bad point number is named
    with pytest.raises(ValueError, match="point %d of the part" % k):
        engine.commit_points_add(*_split(bad, chunks, held))
    assert engine.commit_points_count() == 1
    assert engine.commit_points_add(*_split(good[::-1], chunks, held)) == 1
    assert _got(engine.commit_points_sum(np.array([0]))) == good
    pair = _got(engine.commit_points_sum(np.array([1, 0])))
    assert pair == [C.marshal(C.add(C.unmarshal(a), C.unmarshal(b))) for a, b in zip(good, good[::-1])]


def test_chain_from_the_clients_commitments():
    """Three clients' bk_commit_generate outputs with miner 1's witnesses, summed:
    the commitments are those of the summed update, the witnesses the oracle's sums."""
    from biscotti_amd.krum import Engine
    import shares_ref as S
    eng = Engine(0)
    try:
        eng.commit_set_key(C.key_bytes(C.key_powers(25)))
        rng = np.random.default_rng(28)
        qs = [np.array(S.quantize(rng.normal(0.0, 0.1, size=25), 4), dtype=np.int64) for _ in range(3)]
        store = commit.PointStore(3, 5, 3, engine=eng)
        mine = []
        for i, q in enumerate(qs):
            com, chk, wit = eng.commit_generate(q, 4, 10, 20)
            mine.append(wit[:, 5:10])
            store.add_part(i, com, chk, mine[-1])
        com, chk, wit = store.miner_points([2, 0, 1])
        tcom, tchk, _ = eng.commit_generate(qs[0] + qs[1] + qs[2], 4, 10, 20)
        assert com.tobytes() == tcom.tobytes() and chk.tobytes() == tchk.tobytes()
        for c in range(3):
            for j in range(5):
                rows = [[C.unmarshal(m[c, j])] for m in mine]
                assert wit[c, j].tobytes() == _fold(rows)[0], (c, j)
    finally:
        eng.close()
