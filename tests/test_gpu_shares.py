"""MI355X: the secure-aggregation shares (bk_shares_*) bit for bit against the
pure-Python reference (tests/shares_ref.py) and against the engine's own
quantised sum of the same deltas.

d = 2,561 gives 257 chunks (past one 256-thread workgroup, ending in a chunk of
one coefficient); each d runs with (total shares, miners) = (20, 1), (21, 3),
(20, 4) and with pageable, pinned and device inputs.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import shares_ref as R  # noqa: E402
from biscotti_amd import _lib  # noqa: E402

H, PIN, DEV = _lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE
WHERES = {"host": H, "pinned": PIN, "device": DEV}
P, PREC = 10, 4
DS = [1, 10, 25, 2561, 7850]
LAYOUTS = [(20, 1), (21, 3), (20, 4)]
CLIENTS = 5


@functools.lru_cache(maxsize=None)
def _deltas(d):
    return np.random.default_rng(4000 + d).normal(0.0, 0.1, size=(CLIENTS, d))


@functools.lru_cache(maxsize=None)
def _large(d):
    """Entries up to 1e11 with NaN and +-inf among them: INT64_MIN terms and a
    non-zero correction."""
    rng = np.random.default_rng(5000 + d)
    v = rng.uniform(-1e11, 1e11, size=d)
    for i, x in zip(range(0, d, 7), [np.nan, np.inf, -np.inf, 1e300, -0.0] * d):
        v[i] = x
    return v


@functools.lru_cache(maxsize=None)
def _ref(kind, d, T):
    v = _deltas(d)[0] if kind == "small" else _large(d)
    return R.generate(v, PREC, P, T)


class Buf:
    """A numpy array's content at `where`, with its pointer; host() reads it back."""

    def __init__(self, a, where):
        a = np.ascontiguousarray(a)
        self.where, self.shape, self.dtype = where, a.shape, a.dtype
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
        if self.where == H:
            return self.t
        return self.t.cpu().numpy()


def _generate(engine, v, T, where):
    chunks = -(-v.shape[0] // P)
    src = Buf(v, where)
    dst = Buf(np.zeros((chunks, T), dtype=np.int64), where)
    engine.shares_generate_ptr(src.ptr, where, v.shape[0], PREC, P, T, dst.ptr)
    return dst.host().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _qsum(engine, X):
    """The engine's existing quantised sum (k_qsum) of all rows of X and its
    float form."""
    n, d = X.shape
    dx = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    s = torch.empty(d, dtype=torch.int64, device="cuda")
    sf = torch.empty(d, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    engine.quantized_sum_ptr(dx.data_ptr(), _lib.BK_F64, n, d, d, idx.data_ptr(), n, PREC,
                             s.data_ptr(), sf.data_ptr())
    engine.synchronize()
    return s.cpu().numpy(), sf.cpu().numpy()


def _recover(engine, parts, xs, w, where, own=None):
    """bk_shares_recover through the raw-pointer wrapper with everything at
    `where`; own: the index of the part taken from the context's aggregate."""
    d = w.shape[0]
    keep = [None if i == own else Buf(p, where) for i, p in enumerate(parts)]
    ptrs = (ctypes.c_void_p * len(parts))(*[b.ptr if b is not None else None for b in keep])
    held = np.array([p.shape[1] for p in parts], dtype=np.intc)
    wb = Buf(w, where)
    coef = Buf(np.full(d, -7, dtype=np.int64), where)
    delta = Buf(np.full(d, -7.0), where)
    out = Buf(np.full(d, -7.0), where)
    bad = engine.shares_recover_ptr(ptrs, held, np.ascontiguousarray(xs, dtype=np.int64), where, d,
                                    P, PREC, wb.ptr, coef.ptr, delta.ptr, out.ptr)
    return coef.host().copy(), delta.host().copy(), out.host().copy(), bad


@pytest.mark.parametrize("where", list(WHERES))
@pytest.mark.parametrize("T,miners", LAYOUTS)
@pytest.mark.parametrize("d", DS)
def test_generation_is_the_reference_bit_for_bit(engine, d, T, miners, where):
    before = engine.shares_stats()
    for kind, v in (("small", _deltas(d)[0]), ("large", _large(d))):
        got = _generate(engine, v, T, WHERES[where])
        want = _ref(kind, d, T)
        assert got.shape == want.shape and np.array_equal(got, want), kind
    if d >= 10:
        # the large vector does exercise the conversion's indefinite value and the correction
        q = R.quantize(_large(d)[:P], PREC)
        assert R.INT64_MIN in q
    after = engine.shares_stats()
    assert after[0] - before[0] == 2 and after[2] - before[2] == 2


def test_generate_wrapper_and_miner_split(engine):
    from biscotti_amd import shares
    v = _deltas(25)[1]
    parts = shares.generate_miner_shares(v, 4, engine=engine)
    want = R.generate(v, PREC, P, 20)
    assert len(parts) == 4
    for m, p in enumerate(parts):
        assert p.shape == (3, 5) and np.array_equal(p, want[:, 5 * m:5 * m + 5])
        assert np.array_equal(shares.miner_nodes(m, 5), np.arange(5 * m, 5 * m + 5) - 10)


@pytest.mark.parametrize("d,held", [(25, 5), (25, 20), (10, 7), (2561, 5)])
def test_sum_is_numpys_wrapping_sum(engine, d, held):
    chunks = -(-d // P)
    rng = np.random.default_rng(77 + d + held)
    parts = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=(35, chunks, held),
                         dtype=np.int64, endpoint=True)
    engine.shares_begin(d, P, held, 35)
    for i, p in enumerate(parts):
        assert engine.shares_add(p) == i
    assert engine.shares_count() == 35
    perm = rng.permutation(35)
    for slots in (perm[:1], perm[:5], perm, np.sort(perm[:5]), np.arange(35)[::2]):
        before = engine.shares_stats()
        got = engine.shares_sum(slots)
        assert np.array_equal(got, R.wrapping_sum([parts[s] for s in slots]))
        assert engine.shares_stats()[0] - before[0] == 1
    with pytest.raises(ValueError, match="listed twice"):
        engine.shares_sum(np.array([3, 4, 3]))
    with pytest.raises(ValueError, match=r"slots\[1\]=35"):
        engine.shares_sum(np.array([0, 35]))
    with pytest.raises(ValueError):
        engine.shares_sum(np.array([], dtype=np.int64))


def _miner_sums(engine, d, T, miners):
    """Generate every client's shares, split them by miner, add and sum per
    miner: the miners' aggregates (the last one is left as the context's own)."""
    held = T // miners
    client_parts = []
    for v in _deltas(d):
        y = engine.shares_generate(v, PREC, P, T)
        client_parts.append([np.ascontiguousarray(y[:, held * m:held * (m + 1)])
                             for m in range(miners)])
    sums = []
    for m in range(miners):
        engine.shares_begin(d, P, held, CLIENTS)
        for cp in client_parts:
            engine.shares_add(cp[m])
        s = engine.shares_sum(np.arange(CLIENTS))
        assert np.array_equal(s, R.wrapping_sum([cp[m] for cp in client_parts]))
        sums.append(s)
    xs = np.arange(T, dtype=np.int64) - R.X0
    return sums, xs, held


@pytest.mark.parametrize("where", list(WHERES))
@pytest.mark.parametrize("T,miners", LAYOUTS)
@pytest.mark.parametrize("d", DS)
def test_pipeline_recovers_the_quantised_sum(engine, d, T, miners, where):
    sums, xs, held = _miner_sums(engine, d, T, miners)
    w = np.random.default_rng(6000 + d).normal(size=d)
    want_q, want_f = _qsum(engine, _deltas(d))
    before = engine.shares_stats()
    coef, delta, out, bad = _recover(engine, sums, xs, w, WHERES[where])
    after = engine.shares_stats()
    assert bad == 0 and after[0] - before[0] == 1 and after[3] == before[3]
    assert np.array_equal(coef, want_q)
    assert np.array_equal(_bits(delta), _bits(want_f))
    assert np.array_equal(_bits(out), _bits(w + want_f))
    # one part from the context's own aggregate (the last miner's sum)
    c2, d2, o2, bad2 = _recover(engine, sums, xs, w, WHERES[where], own=miners - 1)
    assert bad2 == 0 and np.array_equal(c2, coef)
    assert np.array_equal(_bits(d2), _bits(delta)) and np.array_equal(_bits(o2), _bits(out))
    if miners == 4:
        # one of four miners missing: shares 0-4 and 10-19
        keep = [0, 2, 3]
        xs3 = np.concatenate([xs[held * m:held * (m + 1)] for m in keep])
        c3, d3, o3, bad3 = _recover(engine, [sums[m] for m in keep], xs3, w, WHERES[where])
        assert bad3 == 0 and np.array_equal(c3, coef)
        assert np.array_equal(_bits(d3), _bits(delta)) and np.array_equal(_bits(o3), _bits(out))


@pytest.mark.parametrize("d", DS)
def test_recovery_is_the_float_methods_result(engine, d):
    sums, xs, _ = _miner_sums(engine, d, 20, 4)
    w = np.zeros(d)
    g, coef, delta, bad = engine.shares_recover(w, sums, xs, PREC, P)
    assert bad == 0
    y = np.concatenate(sums, axis=1)
    chunks = y.shape[0]
    for c in sorted({0, 1, chunks // 2, chunks - 2, chunks - 1} & set(range(chunks))):
        rounded, sol = R.recover_float(xs, y[c], P)
        assert np.max(np.abs(sol - np.rint(sol))) < 0.25
        n = min(P, d - c * P)
        assert np.array_equal(coef[c * P:c * P + n], rounded[:n])
        assert not rounded[n:].any()


@pytest.mark.parametrize("d,chunk,share", [(25, 1, 0), (25, 2, 19), (2561, 255, 9), (2561, 256, 12),
                                           (7850, 400, 10)])
def test_an_altered_share_zeroes_its_chunk_only(engine, d, chunk, share):
    sums, xs, held = _miner_sums(engine, d, 20, 4)
    w = np.random.default_rng(d).normal(size=d)
    g0, c0, f0, bad0 = engine.shares_recover(w, sums, xs, PREC, P)
    assert bad0 == 0
    alt = [s.copy() for s in sums]
    alt[share // held][chunk, share % held] += 1
    before = engine.shares_stats()
    g1, c1, f1, bad1 = engine.shares_recover(w, alt, xs, PREC, P)
    assert bad1 == 1 and engine.shares_stats()[3] - before[3] == 1
    lo, hi = chunk * P, min(d, chunk * P + P)
    assert not c1[lo:hi].any() and not f1[lo:hi].any()
    assert np.array_equal(_bits(g1[lo:hi]), _bits(w[lo:hi] + 0.0))
    for a, b in ((c0, c1), (f0, f1), (g0, g1)):
        assert np.array_equal(_bits(np.delete(a, np.s_[lo:hi])), _bits(np.delete(b, np.s_[lo:hi])))
    assert c0[lo:hi].any()


def test_store_and_recover_wrappers(engine):
    from biscotti_amd import shares
    d, T, miners = 25, 20, 4
    held = shares.shares_per_miner(T, miners)
    per_client = [shares.generate_miner_shares(v, miners, engine=engine) for v in _deltas(d)]
    w = np.random.default_rng(1).normal(size=d)
    replies = []
    for m in range(miners):
        store = shares.ShareStore(d, held, CLIENTS, engine=engine)
        for node, parts in enumerate(per_client):
            store.add_part(100 + node, parts[m])
        with pytest.raises(ValueError):
            store.add_part(100, per_client[0][m])
        replies.append(store.miner_part([100 + n for n in range(CLIENTS)]))
    xs = np.concatenate([shares.miner_nodes(m, held) for m in range(miners)])
    g, delta, bad = shares.recover_block(w, replies[:-1] + [None], xs, engine=engine)
    want_q, want_f = _qsum(engine, _deltas(d))
    assert bad == 0 and np.array_equal(_bits(delta), _bits(want_f))
    assert np.array_equal(_bits(g), _bits(w + want_f))
