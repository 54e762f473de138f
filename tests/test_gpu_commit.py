"""MI355X: the bn256 G1 commitments (bk_commit_*) against the pure-Python oracle
(tests/commit_ref.py), all 64 bytes of every point.

Two keys: PK[i] = 2^i G (GenerateKey's own shape), and a crafted one with
PK[1] = PK[0], PK[2] = -PK[0], PK[5] infinity and random multiples of G
elsewhere, on which equal scalars meet the doubling inside an addition and
opposite terms pass through infinity in mid-sum.  d = 2,561 (257 chunks, past one
workgroup, the last chunk of one coefficient) is compared with the goldens of
tests/golden/gen_commit_goldens.py.
"""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import commit_ref as C  # noqa: E402
import shares_ref as S  # noqa: E402
from biscotti_amd import _lib  # noqa: E402

H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
WHERES = {"host": H, "pinned": PIN, "device": DEV}
P, PREC = 10, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "commit_d2561.npz")
EDGE = (list(range(-33, 34)) + [(1 << 63) - 1, S.INT64_MIN, 1 << 32, -(1 << 32), (1 << 60) + 1,
                                -((1 << 60) + 1)])


@functools.lru_cache(maxsize=None)
def _powers():
    key = C.key_powers(2561)
    return key, C.key_bytes(key)


@functools.lru_cache(maxsize=None)
def _crafted():
    rng = random.Random(99)
    key = [C.mul(C.G, rng.randrange(1, C.N)) for _ in range(16)]
    key[1] = key[0]
    key[2] = C.neg(key[0])
    key[5] = C.INF
    return key, C.key_bytes(key)


_current = [None]


def _use(engine, which):
    """Make the named key the engine's resident key (once per change)."""
    key, raw = _powers() if which == "powers" else _crafted()
    if _current[0] != which:
        engine.commit_set_key(raw)
        _current[0] = which
        assert engine.commit_key_count() == len(key) == engine.commit_stats()[3]
    return key


class Buf:
    """A numpy array's content at `where`, with its pointer; host() reads it back."""

    def __init__(self, a, where):
        a = np.ascontiguousarray(a)
        self.where = where
        if where == H:
            self.t = a.copy()
            self.ptr = self.t.ctypes.data
        elif where == PIN:
            self.t = torch.from_numpy(a.copy()).pin_memory()
            self.ptr = self.t.data_ptr()
        else:
            self.t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            self.ptr = self.t.data_ptr()

    def host(self):
        return self.t if self.where == H else self.t.cpu().numpy()


def _msm(engine, scalars, first, where):
    src = Buf(np.asarray(scalars, dtype=np.int64), where)
    dst = Buf(np.full(64, 0xAB, dtype=np.uint8), where)
    engine.commit_msm_ptr(src.ptr, where, len(scalars), first, dst.ptr)
    return dst.host().tobytes()


@functools.lru_cache(maxsize=None)
def _msm_case(n, first):
    """Scalars of every size, both signs, zeros among them; and the oracle's sum."""
    rng = random.Random(1000 * n + first)
    sc = []
    for i in range(n):
        bits = (1, 4, 8, 16, 33, 63)[i % 6]
        v = rng.randrange(1 << bits)
        sc.append(0 if i % 11 == 7 else (-v if rng.random() < 0.5 else v))
    key = _powers()[0]
    return sc, C.marshal(C.commit_fast(sc, key[first:first + n]))


@pytest.mark.parametrize("where", list(WHERES))
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 10, 11, 257])
def test_msm_lengths_and_placement(engine, n, first, where):
    _use(engine, "powers")
    sc, want = _msm_case(n, first)
    before = engine.commit_stats()
    assert _msm(engine, sc, first, WHERES[where]) == want
    after = engine.commit_stats()
    assert after[0] - before[0] == 1 and after[2] - before[2] == 1
    assert after[1] - before[1] == (0 if where == "device" else 2)


def test_msm_edge_scalars(engine):
    key = _use(engine, "crafted")
    pt = key[3]
    for v in EDGE:
        assert _msm(engine, [v], 3, H) == C.marshal(C.mul_fast(pt, v)), v
    # all of them in one sum
    key = _use(engine, "powers")
    assert _msm(engine, EDGE, 3, H) == C.marshal(C.commit_fast(EDGE, key[3:3 + len(EDGE)]))
    assert engine.commit_msm(np.array(EDGE, dtype=np.int64), first=3) == \
        C.marshal(C.commit_fast(EDGE, key[3:3 + len(EDGE)]))


def test_msm_zero_doubling_and_infinity(engine):
    key = _use(engine, "crafted")
    for where in (H, DEV):
        assert _msm(engine, [0] * 16, 0, where) == C.ZERO64
    cases = [
        [7, 7],                        # equal points: the doubling inside an addition
        [S.INT64_MIN, S.INT64_MIN],
        [9, 0, 9],                     # 9 P - 9 P: infinity in mid-sum, alone
        [9, 0, 9, 5, -3, 4, 1],        # ... and with terms after it (PK[5] is infinity)
        [-8, 8, 8, 0, 0, 1 << 40],
        [3, 3, 6],                     # 3 P + 3 P - 6 P = infinity
        [0, 0, 0, 0, 0, 12345],        # a scalar on the infinity entry
        list(range(-8, 8)),
    ]
    for sc in cases:
        assert _msm(engine, sc, 0, H) == C.marshal(C.commit_fast(sc, key[:len(sc)])), sc
    assert _msm(engine, [3, 3, 6], 0, H) == C.ZERO64
    # the same meetings inside one thread's walk (a chunk's terms share a thread)
    for sc in cases:
        q = np.array(sc, dtype=np.int64)
        _, chk, wit = engine.commit_generate(q, PREC, P, 20, want_commit=False)
        _, cc, ww = C.generate(sc, key, P, 20)
        assert chk.tobytes() == b"".join(cc), sc
        assert wit.tobytes() == b"".join(b"".join(r) for r in ww.values()), sc


def _deltas(d):
    return np.random.default_rng(4000 + d).normal(0.0, 0.1, size=d)


def _large(d):
    """tests/test_gpu_shares.py's _large: INT64_MIN terms among entries up to 1e15."""
    rng = np.random.default_rng(5000 + d)
    v = rng.uniform(-1e11, 1e11, size=d)
    for i, x in zip(range(0, d, 7), [np.nan, np.inf, -np.inf, 1e300, -0.0] * d):
        v[i] = x
    return v


@functools.lru_cache(maxsize=None)
def _gen_ref(kind, d, T):
    v = _deltas(d) if kind == "small" else _large(d)
    q = S.quantize(v, PREC)
    whole, cc, ww = C.generate(q, _powers()[0], P, T)
    return (v, np.array(q, dtype=np.int64), whole, b"".join(cc),
            b"".join(b"".join(ww[c]) for c in range(len(cc))))


def _generate(engine, src, where, d, T, want=(True, True, True)):
    chunks = -(-d // P)
    is_q = src.dtype == np.int64
    sb = Buf(src, where)
    outs = [Buf(np.full(n, 0xCD, dtype=np.uint8), where) if w else None
            for n, w in zip((64, chunks * 64, chunks * T * 64), want)]
    engine.commit_generate_ptr(None if is_q else sb.ptr, sb.ptr if is_q else None, where, d, PREC, P,
                               T, *[o.ptr if o else None for o in outs])
    return [o.host().tobytes() if o else None for o in outs]


@pytest.mark.parametrize("src", ["delta", "q"])
@pytest.mark.parametrize("T", [20, 21])
@pytest.mark.parametrize("d", [1, 10, 11, 25])
def test_generate_shapes(engine, d, T, src):
    _use(engine, "powers")
    v, q, whole, cc, ww = _gen_ref("small", d, T)
    where = DEV if (d + T) % 2 else H
    before = engine.commit_stats()
    got = _generate(engine, v if src == "delta" else q, where, d, T)
    after = engine.commit_stats()
    assert got[0] == whole and got[1] == cc and got[2] == ww
    assert after[0] - before[0] == 3 and after[2] - before[2] == 1
    if d == 1:
        assert ww == bytes(64 * T)
    # each output alone is the output requested with the others
    for i in range(3):
        want = tuple(j == i for j in range(3))
        alone = _generate(engine, v if src == "delta" else q, where, d, T, want)
        assert alone[i] == got[i] and [a is None for a in alone] == [not w for w in want]


def test_generate_large_entries(engine):
    _use(engine, "powers")
    v, q, whole, cc, ww = _gen_ref("large", 25, 20)
    assert S.INT64_MIN in q.tolist()
    for where in (H, DEV):
        assert _generate(engine, v, where, 25, 20) == [whole, cc, ww]
    assert _generate(engine, q, PIN, 25, 20) == [whole, cc, ww]


def test_generate_2561_against_the_goldens(engine):
    _use(engine, "powers")
    g = np.load(GOLDEN)
    d, p, T, prec = g["params"].tolist()
    assert (d, p, T, prec) == (2561, P, 20, PREC)
    assert np.array_equal(np.array(S.quantize(g["delta"], PREC), dtype=np.int64), g["q"])
    com, chk, wit = engine.commit_generate(g["delta"], PREC, P, T)
    assert chk.shape == (257, 64) and wit.shape == (257, 20, 64)
    assert np.array_equal(com, g["commit"])
    assert np.array_equal(chk, g["chunk"])
    for i, c in enumerate(g["witness_chunks"].tolist()):
        assert np.array_equal(wit[c], g["witness"][i]), c
    assert not wit[256].any()  # one coefficient: an empty quotient
    com2, chk2, wit2 = engine.commit_generate(g["q"], PREC, P, T)
    assert np.array_equal(com, com2) and np.array_equal(chk, chk2) and np.array_equal(wit, wit2)
    # the module's surface on the same key
    from biscotti_amd import commit
    key = commit.CommitKey(engine, engine.commit_key_count())
    assert len(key) == 2561
    assert commit.create_commitment(key, g["q"]) == g["commit"].tobytes()
    a, b, c = commit.generate_miner_commitments(key, g["delta"][:25])
    assert a.shape == (64,) and b.shape == (3, 64) and c.shape == (3, 20, 64)
    assert np.array_equal(b[:2], g["chunk"][:2]) and np.array_equal(c[0], g["witness"][0])


def test_verify(engine):
    key = _use(engine, "powers")
    sc, want = _msm_case(11, 3)
    s = np.array(sc, dtype=np.int64)
    assert engine.commit_verify(s, want, first=3) is True
    off = s.copy()
    off[4] += 1
    assert engine.commit_verify(off, want, first=3) is False
    for byte in (0, 31, 63):
        bad = bytearray(want)
        bad[byte] ^= 1
        assert engine.commit_verify(s, bytes(bad), first=3) is False
    assert engine.commit_verify(s, want, first=0) is False
    # device placement of the scalars and of the committed point
    ok = ctypes.c_int(-1)
    sb, cb = Buf(s, DEV), Buf(np.frombuffer(want, dtype=np.uint8), DEV)
    assert _lib.lib().bk_commit_verify(engine._ctx, sb.ptr, DEV, 11, 3, cb.ptr,
                                       ctypes.byref(ok)) == _lib.BK_OK
    assert ok.value == 1
    assert engine.commit_verify(np.zeros(4, dtype=np.int64), C.ZERO64) is True
    del key


def test_key_errors_leave_the_key(engine):
    key = _use(engine, "crafted")
    raw = bytearray(_crafted()[1])
    sc = [5, -6, 7, 8]
    want = C.marshal(C.commit_fast(sc, key[:4]))
    off = bytearray(raw)
    off[64 * 9 + 40] ^= 4                       # point 9 off the curve
    big = bytearray(raw)
    big[64 * 4:64 * 4 + 32] = C.P.to_bytes(32, "big")   # point 4: x = p
    ff = bytearray(raw)
    ff[64 * 7 + 32:64 * 8] = b"\xff" * 32       # point 7: y = 2^256 - 1
    both = bytearray(off)
    both[64 * 12] ^= 1                          # the smallest index is named
    # the binding raises ValueError for BK_EINVAL (biscotti_amd/_lib.py check)
    for bad, idx in ((off, 9), (big, 4), (ff, 7), (both, 9)):
        buf = np.frombuffer(bytes(bad), dtype=np.uint8)
        assert _lib.lib().bk_commit_set_key(engine._ctx, buf.ctypes.data, 16) == _lib.BK_EINVAL
        assert "key point %d " % idx in _lib.last_error()
        with pytest.raises(ValueError) as ei:
            engine.commit_set_key(bytes(bad))
        assert "key point %d " % idx in str(ei.value)
        assert engine.commit_key_count() == 16
        assert _msm(engine, sc, 0, H) == want
    with pytest.raises(ValueError, match="past the key"):
        _msm(engine, [1] * 17, 0, H)
    with pytest.raises(ValueError, match="past the key"):
        _msm(engine, [1] * 4, 13, H)
    with pytest.raises(ValueError, match="past the key"):
        _generate(engine, np.zeros(17), H, 17, 20)
    assert _msm(engine, sc, 0, H) == want


def test_chain_with_the_gradient_step(engine):
    """q_out of bk_grad_logistic left on the device feeds bk_commit_generate."""
    _use(engine, "powers")
    rng = np.random.default_rng(26)
    nn, d = 64, 25
    X = rng.normal(size=(nn, d))
    y = np.where(rng.random(nn) < 0.5, -1.0, 1.0)
    ww = rng.normal(0.0, 0.1, size=d)
    engine.grad_set_logistic(X, y)
    try:
        wb = Buf(ww, DEV)
        delta = Buf(np.zeros(d), DEV)
        q = Buf(np.zeros(d, dtype=np.int64), DEV)
        engine.grad_logistic_ptr(wb.ptr, DEV, None, 10, 1e-2, 0.01, None, PREC, delta.ptr, q.ptr)
        outs = [Buf(np.zeros(n, dtype=np.uint8), DEV) for n in (64, 3 * 64, 3 * 20 * 64)]
        engine.commit_generate_ptr(None, q.ptr, DEV, d, PREC, P, 20, *[o.ptr for o in outs])
        chained = [o.host().tobytes() for o in outs]
        # the host route: the same step's outputs fetched, then committed from the host
        hq, hdelta = q.host().copy(), delta.host().copy()
        assert np.array_equal(hq, np.array(S.quantize(hdelta, PREC), dtype=np.int64))
        assert hq.any()
        com, chk, wit = engine.commit_generate(hq, PREC, P, 20)
        assert chained == [com.tobytes(), chk.tobytes(), wit.tobytes()]
        com2, _, _ = engine.commit_generate(hdelta, PREC, P, 20)
        assert com2.tobytes() == chained[0]
        assert chained[0] == C.marshal(C.commit_fast(hq.tolist(), _powers()[0][:d]))
    finally:
        engine.grad_clear()
