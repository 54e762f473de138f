"""bk_multikrum_ragged*: B independent Multi-Krum problems in one call, every
problem with its own rows, its own n and its own f (k_small_ragged /
k_tiny_ragged, bk_small_ragged.hip; the single device path for a group's only
problem and outside their range).

The bar, in every case: sel, scores, mean and the eight margin fields of every
problem are BITWISE what bk_multikrum_device gives on that problem alone on the
same engine (a NaN matches a NaN), and the selection is the oracle's wherever
the problem's record says near_tie = 0.  No tolerance appears anywhere."""
import ctypes
import os

import numpy as np
import pytest

import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

CHAIN = ("k_scores", "k_rank", "k_compact")  # K2, K3, K3b as bk_timing_read names them
ONE = "k_small"  # BK_K_SMALL: the ragged launches and the single one-launch calls
PAD = 777.25     # fills the gaps between rows: never read
GUARD = 5        # untouched elements behind every packed output


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    """bitwise, a NaN matching a NaN (test_gpu_batch.py's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return (a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and
            np.array_equal(_bits(a[~nan]), _bits(b[~nan])))


def _record(engine):
    rec = (ctypes.c_double * 8)()
    _lib.check(_lib.lib().bk_selection_margin_record(engine.ctx, rec))
    return np.array(list(rec), dtype=np.float64)


def _records(engine, B):
    rec = (ctypes.c_double * (8 * B))()
    _lib.check(_lib.lib().bk_selection_margin_batch(engine.ctx, rec, B))
    return np.array(list(rec), dtype=np.float64).reshape(B, 8)


def _problem(n, d, seed, dtype=np.float64):
    """a seeded problem: a common drift, a few far-off rows"""
    rng = np.random.default_rng(seed)
    P = 0.01 * (1 + seed % 5) * rng.standard_normal(d) + 1e-3 * rng.standard_normal((n, d))
    far = rng.choice(n, size=max(1, n // 4), replace=False)
    P[far] += 0.05 * rng.standard_normal((far.size, d))
    return P.astype(dtype)


def _f_choices(n):
    """{1, n // 2, n - 2 (k = 0), n - 1 (m = 1)} where valid (1 <= f < n)"""
    return sorted({f for f in (1, n // 2, n - 2, n - 1) if 1 <= f < n})


def _mix(ns, d, seed, dtype=np.float64):
    """problems of the sizes ns (in that order), f cycling through each size's choices"""
    probs = [_problem(n, d, seed + 31 * b, dtype) for b, n in enumerate(ns)]
    fs = [_f_choices(n)[b % len(_f_choices(n))] for b, n in enumerate(ns)]
    return probs, fs


class Pack:
    """the problems packed in ONE row-major device matrix: row stride ld, the
    base `off` elements past the allocation, PAD between the rows"""

    def __init__(self, probs, ld=None, off=0):
        self.probs = probs
        self.B = len(probs)
        self.d = probs[0].shape[1]
        self.ld = ld or self.d
        self.off = off
        self.es = probs[0].itemsize
        self.dt = _lib.BK_F32 if probs[0].dtype == np.float32 else _lib.BK_F64
        self.ns = np.array([p.shape[0] for p in probs], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        rows = int(self.offsets[-1])
        flat = np.full(off + (rows - 1) * self.ld + self.d, PAD, dtype=probs[0].dtype)
        for b, p in enumerate(probs):
            for i in range(p.shape[0]):
                s = off + (int(self.offsets[b]) + i) * self.ld
                flat[s:s + self.d] = p[i]
        self.buf = torch.from_numpy(flat).cuda()

    def ptr(self, b=0):
        return self.buf.data_ptr() + (self.off + int(self.offsets[b]) * self.ld) * self.es


def _singles(engine, K, fs):
    """bk_multikrum_device on each problem alone -> [(sel, scores, mean, record)]"""
    out = []
    for b in range(K.B):
        n, f = int(K.ns[b]), int(fs[b])
        sel = torch.full((n - f,), -7, dtype=torch.int64, device="cuda")
        sc = torch.full((n,), PAD, dtype=torch.float64, device="cuda")
        mean = torch.full((K.d,), PAD, dtype=torch.float64, device="cuda")
        engine.multikrum_device_ptr(K.ptr(b), K.dt, n, K.d, K.ld, f, sel.data_ptr(),
                                    sc.data_ptr(), mean.data_ptr())
        rec = _record(engine)
        out.append((sel.cpu().numpy(), sc.cpu().numpy(), mean.cpu().numpy(), rec))
    return out


class Outs:
    """device outputs of one ragged call, packed as the header says, with GUARD
    elements behind each that the call must leave alone"""

    def __init__(self, K, fs, ws=True, wm=True):
        self.K, self.fs = K, np.asarray(fs, dtype=np.int64)
        self.ms = K.ns - self.fs
        self.so = np.concatenate([[0], np.cumsum(self.ms)]).astype(np.int64)
        self.sel = torch.full((int(self.so[-1]) + GUARD,), -7, dtype=torch.int64, device="cuda")
        self.sc = (torch.full((int(K.offsets[-1]) + GUARD,), PAD, dtype=torch.float64,
                              device="cuda") if ws else None)
        self.mean = (torch.full((K.B * K.d + GUARD,), PAD, dtype=torch.float64, device="cuda")
                     if wm else None)

    def launch(self, engine):
        K = self.K
        engine.multikrum_ragged_device_ptr(
            K.ptr(0), K.dt, K.offsets, self.fs, K.d, K.ld, self.sel.data_ptr(),
            self.sc.data_ptr() if self.sc is not None else None,
            self.mean.data_ptr() if self.mean is not None else None)

    def read(self, recs):
        """[(sel, scores, mean, record)] per problem; the guards are checked"""
        K = self.K
        sel = self.sel.cpu().numpy()
        assert (sel[int(self.so[-1]):] == -7).all(), "sel guard"
        sc = mean = None
        if self.sc is not None:
            sc = self.sc.cpu().numpy()
            assert (sc[int(K.offsets[-1]):] == PAD).all(), "scores guard"
        if self.mean is not None:
            mean = self.mean.cpu().numpy()
            assert (mean[K.B * K.d:] == PAD).all(), "mean guard"
        return [(sel[self.so[b]:self.so[b + 1]],
                 sc[K.offsets[b]:K.offsets[b + 1]] if sc is not None else None,
                 mean[b * K.d:(b + 1) * K.d] if mean is not None else None,
                 recs[b]) for b in range(K.B)]


def _ragged(engine, K, fs, ws=True, wm=True):
    o = Outs(K, fs, ws, wm)
    o.launch(engine)
    engine.synchronize()
    return o.read(_records(engine, K.B))


def _pick(recs):
    """the record bk_selection_margin* reports after a batched call"""
    recs = np.asarray(recs)
    near = np.flatnonzero(recs[:, 2] != 0)
    if near.size:
        return recs[near[0]]
    return recs[np.argmin(recs[:, 0] - recs[:, 1])]


def _assert_bitwise(got, ref, what):
    assert len(got) == len(ref), what
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g[0].dtype == np.int64 and np.array_equal(g[0], r[0]), (what, b, "sel", g[0], r[0])
        if g[1] is not None:
            assert _same(g[1], r[1]), (what, b, "scores")
        if g[2] is not None:
            assert _same(g[2], r[2]), (what, b, "mean")
        assert _same(g[3], r[3]), (what, b, "margin", g[3], r[3])


def _assert_oracle(oracle, K, fs, got, what, skip=()):
    for b, g in enumerate(got):
        if g[3][2] == 0 and b not in skip:
            want = oracle.krum(np.ascontiguousarray(K.probs[b]), int(fs[b]), False, False)[0]
            assert np.array_equal(g[0], want), (what, b)


def _timed(engine, call):
    engine.timing_enable(True)
    try:
        out = call()
        return out, engine.timing_read()
    finally:
        engine.timing_enable(False)


def _check(engine, oracle, K, fs, what, ref=None, skip=()):
    ref = ref or _singles(engine, K, fs)
    got = _ragged(engine, K, fs)
    _assert_bitwise(got, ref, what)
    _assert_oracle(oracle, K, fs, got, what, skip)
    assert _same(_record(engine), _pick([g[3] for g in got])), what
    return got, ref


# every NB = ceil(n / 16) from 1 to 8 but 6, shuffled so the groups interleave in
# the caller's order; NB = 4 (n = 64) is a deliberate singleton -- the single
# path inside the same call -- and every other group has two problems or more
MAIN_NS = [2, 3, 10, 16, 17, 31, 32, 33, 48, 64, 65, 100, 113, 128,
           3, 16, 17, 32, 48, 65, 100, 113, 128, 10]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d", [130, 257, 1000])
def test_main_mix(engine, oracle, d, dtype):
    """d = 130: P = 2 chunks; 257: P = 3, the odd half-split of the partials;
    1,000: 8 chunks, 16 M items.  24 problems, 6 groups and a singleton"""
    ns = list(np.random.default_rng(5).permutation(MAIN_NS))
    assert sum(1 for n in ns if (n + 15) // 16 == 4) == 1
    probs, fs = _mix(ns, d, 400 + d, dtype)
    K = Pack(probs)
    (got, _), t = _timed(engine, lambda: _check(engine, oracle, K, fs, (d, dtype)))
    # 24 singles, then the ragged call: 6 launches and the singleton's own
    assert t[ONE]["count"] == 24 + 6 + 1 and not any(k in t for k in CHAIN), t
    # every f kind is there: k = 0 (f = n - 2), m = 1 (f = n - 1)
    assert any(f == n - 2 for n, f in zip(ns, fs)) and any(f == n - 1 for n, f in zip(ns, fs))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_tiny_group(engine, oracle, dtype):
    """d = 25: the NB = 1 group (n = 2..16) runs k_tiny_ragged, one workgroup per
    problem, the n = 17..40 groups k_small_ragged"""
    ns = list(range(2, 17)) + [17, 40, 25, 33, 32, 20]
    ns = list(np.random.default_rng(6).permutation(ns))
    probs, fs = _mix(ns, 25, 77, dtype)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    (got, _), t = _timed(engine, lambda: _check(engine, oracle, K, fs, "tiny", ref))
    assert t[ONE]["count"] == 3, t  # one k_tiny_ragged, NB = 2 and NB = 3


@pytest.mark.parametrize("d", [128, 129])
def test_tiny_edge(engine, oracle, d):
    """d = 128 is k_tiny's last width, 129 the first that takes the queue"""
    ns = [2, 16, 9, 5, 16, 12, 30, 18]
    probs, fs = _mix(ns, d, 91)
    _check(engine, oracle, Pack(probs), fs, d)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,ld,off", [(130, 133, 0), (130, 136, 1), (25, 27, 0), (25, 26, 1)],
                         ids=["odd-ld", "base+1", "tiny-odd-ld", "tiny-base+1"])
def test_layouts(engine, oracle, d, ld, off, dtype):
    """a padded odd ld (scalar loads); an even ld with the base one element past
    the 16-B (fp64) / 8-B (fp32) boundary (scalar loads for every problem).  The
    pad values between the rows are never read: the bits are the packed
    layout's, and the outputs' guards stay (Outs.read)"""
    ns = [17, 10, 33, 32, 5, 48, 20, 16]
    probs, fs = _mix(ns, d, 55, dtype)
    K = Pack(probs, ld=ld, off=off)
    if off:
        assert K.ptr(0) % (2 * K.es) == K.es
    got, _ = _check(engine, oracle, K, fs, (d, ld, off))
    packed = _ragged(engine, Pack(probs), fs)
    _assert_bitwise(packed, got, "packed layout")


def test_more_problems_than_one_launch_holds(engine, oracle):
    """BK_BATCH_WS_BYTES bounds a launch's partials: at NB = 7 and d = 257 a
    problem needs 3 chunks x (112^2 + 112) doubles, so two and a half problems'
    worth makes W = 2, and a group of five runs as launches of 2, 2 and 1"""
    ns = [100, 97, 112, 105, 99, 20, 30]
    probs, fs = _mix(ns, 257, 123)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    per = 3 * (112 * 112 + 112) * 8
    os.environ["BK_BATCH_WS_BYTES"] = str(2 * per + per // 2)
    try:
        got, t = _timed(engine, lambda: _ragged(engine, K, fs))
    finally:
        del os.environ["BK_BATCH_WS_BYTES"]
    assert t[ONE]["count"] == 3 + 1, t  # ... and the NB = 2 group's launch
    _assert_bitwise(got, ref, "W = 2, 2, 1")
    _assert_oracle(oracle, K, fs, got, "W = 2, 2, 1")
    got, t = _timed(engine, lambda: _ragged(engine, K, fs))
    assert t[ONE]["count"] == 2, t
    _assert_bitwise(got, ref, "one launch per group")


def test_n129_among_small_ones(engine, oracle):
    """n = 129 is outside the one-launch range: the chain, inside the same call"""
    ns = [20, 129, 30, 100, 17, 97]
    probs, fs = _mix(ns, 130, 211)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    got, t = _timed(engine, lambda: _ragged(engine, K, fs))
    assert t[ONE]["count"] == 2 and all(t[k]["count"] == 1 for k in CHAIN), t
    _assert_bitwise(got, ref, "n = 129")
    _assert_oracle(oracle, K, fs, got, "n = 129")
    assert _same(_record(engine), _pick([g[3] for g in got]))


def test_wide_rows_whole_call(engine, oracle):
    """d = 40,000 is past the one-launch range for every problem: the loop of
    single device calls"""
    ns = [5, 24, 17]
    probs, fs = _mix(ns, 40000, 311)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    got, t = _timed(engine, lambda: _ragged(engine, K, fs))
    assert ONE not in t and all(t[k]["count"] == 3 for k in CHAIN), t
    _assert_bitwise(got, ref, "d = 40,000")
    _assert_oracle(oracle, K, fs, got, "d = 40,000")


def test_small_path_off(engine, oracle):
    ns = [17, 20, 100, 10]
    probs, fs = _mix(ns, 130, 411)
    K = Pack(probs)
    engine.set_small_path(False)
    try:
        ref = _singles(engine, K, fs)
        got, t = _timed(engine, lambda: _ragged(engine, K, fs))
    finally:
        engine.set_small_path(True)
    assert ONE not in t and all(t[k]["count"] == 4 for k in CHAIN), t
    _assert_bitwise(got, ref, "small path off")
    _assert_oracle(oracle, K, fs, got, "small path off")


@pytest.mark.parametrize("name", ["nan_row", "inf_row", "dup_rows", "edge_zeros_tie",
                                  "edge_n2_f1", "A_n4_k0_tie"])
def test_special_values(name, engine, oracle):
    """a special-value golden as problem 2 of five ordinary ones of other sizes
    (one of them in its group): its neighbours are untouched, it is bitwise its
    single call and selects what the golden does"""
    X, p = GU.build_input(name, oracle)
    X = np.ascontiguousarray(X)
    n, d = X.shape
    ns = [n + 1, 40, n, 33, max(2, n - 1)]
    probs, fs = _mix(ns, d, 7 + n + d, X.dtype)
    probs[2], fs[2] = X, p["f"]
    K = Pack(probs)
    got, _ = _check(engine, oracle, K, fs, name, skip=(2,))  # (the golden holds problem 2's)
    assert np.array_equal(got[2][0], GU.load(name)["sel"]), name


@pytest.mark.parametrize("n,d,f,B", [(100, 257, 30, 7), (10, 25, 2, 40)])
def test_uniform_descriptors(engine, oracle, n, d, f, B):
    """all n and f equal: bitwise bk_multikrum_batch_device's outputs and records"""
    probs = [_problem(n, d, 900 + b) for b in range(B)]
    K = Pack(probs)
    fs = [f] * B
    m = n - f
    sel = torch.full((B * m,), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((B * n,), PAD, dtype=torch.float64, device="cuda")
    mean = torch.full((B * d,), PAD, dtype=torch.float64, device="cuda")
    engine.multikrum_batch_device_ptr(K.ptr(0), K.dt, B, n, d, K.ld, n * K.ld, f, sel.data_ptr(),
                                      sc.data_ptr(), mean.data_ptr())
    engine.synchronize()
    recs = _records(engine, B)
    pick = _record(engine)
    sel, sc, mean = (x.cpu().numpy().reshape(B, -1) for x in (sel, sc, mean))
    ref = [(sel[b], sc[b], mean[b], recs[b]) for b in range(B)]
    got = _ragged(engine, K, fs)
    _assert_bitwise(got, ref, "uniform")
    assert _same(_record(engine), pick)
    _assert_oracle(oracle, K, fs, got, "uniform")


def test_nullable_outputs(engine, oracle):
    ns = [33, 20, 40, 17, 64]
    probs, fs = _mix(ns, 257, 61)
    K = Pack(probs)
    full = _ragged(engine, K, fs)
    for ws, wm in ((True, False), (False, True), (False, False)):
        got = _ragged(engine, K, fs, ws=ws, wm=wm)
        assert all((g[1] is None) == (not ws) and (g[2] is None) == (not wm) for g in got)
        _assert_bitwise(got, full, (ws, wm))
    # the host entry: m_out, scores and mean_out null
    X = np.ascontiguousarray(np.concatenate(probs))
    fa = np.asarray(fs, dtype=np.int64)
    sel = np.full(int((K.ns - fa).sum()), -7, dtype=np.int64)
    _lib.check(_lib.lib().bk_multikrum_ragged(
        engine.ctx, X.ctypes.data, _lib.BK_HOST, K.dt, K.B, K.offsets.ctypes.data, fa.ctypes.data,
        K.d, K.d, sel.ctypes.data, None, None, None))
    assert np.array_equal(sel, np.concatenate([g[0] for g in full]))
    recs = _records(engine, K.B)
    assert all(_same(recs[b], full[b][3]) for b in range(K.B))


def test_host_entry(engine, oracle):
    """from pageable memory (a list of separate arrays, packed by the binding)
    and from pinned memory (views of one pinned matrix, passed as they lie)"""
    ns = [100, 17, 40, 97, 20, 5]
    probs, fs = _mix(ns, 257, 81)
    K = Pack(probs)
    dev = _ragged(engine, K, fs)
    pinned = torch.from_numpy(np.concatenate(probs)).pin_memory().numpy()
    views = [pinned[K.offsets[b]:K.offsets[b + 1]] for b in range(K.B)]
    keys = ("gap", "err_bound", "near_tie", "M", "s_lo", "s_hi", "d", "k")
    for X, pin in ((probs, False), (views, True)):
        out = engine.multikrum_ragged(X, fs, pinned=pin)
        recs = [np.array([r[k] for k in keys], dtype=np.float64)
                for r in engine.selection_margin_batch(K.B)]
        got = [(o[0], o[1], o[2], recs[b]) for b, o in enumerate(out)]
        assert all(o[1].dtype == np.float64 and o[2].shape == (K.d,) for o in out)
        _assert_bitwise(got, dev, ("host", pin))
    out = engine.multikrum_ragged(probs, fs, want_scores=False, want_mean=False)
    assert all(o[1] is None and o[2] is None and np.array_equal(o[0], g[0])
               for o, g in zip(out, dev))


@pytest.mark.parametrize("n,d", [(100, 257), (10, 25), (129, 64)])
def test_batch_of_one(engine, oracle, n, d):
    """batch = 1 is the single call itself: its record is the context's own"""
    probs, fs = _mix([n], d, 19)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    got = _ragged(engine, K, fs)
    _assert_bitwise(got, ref, "batch = 1")
    assert _same(_record(engine), ref[0][3])
    _assert_oracle(oracle, K, fs, got, "batch = 1")


def test_margin_order_and_pick(engine, oracle):
    """bk_selection_margin_batch in the caller's order, and bk_selection_margin's
    pick by the documented rule: the lowest-index near tie (here the all-zero
    golden, placed behind ordinary problems of its own group and of others)"""
    Z, p = GU.build_input("edge_zeros_tie", oracle)
    ns = [40, 9, 33, Z.shape[0], 17, 12]
    probs, _ = _mix(ns, Z.shape[1], 23)
    fs = [10, 3, 8, p["f"], 5, 4]  # k > 0 and m > 1 everywhere: no tie but the golden's
    probs[3] = np.ascontiguousarray(Z)
    K = Pack(probs)
    ref = _singles(engine, K, fs)
    got = _ragged(engine, K, fs)
    _assert_bitwise(got, ref, "records in the caller's order")
    recs = np.array([g[3] for g in got])
    assert recs[3, 2] != 0 and not (recs[:3, 2] != 0).any()
    assert _same(_record(engine), recs[3])
    gap = (ctypes.c_double(), ctypes.c_double(), ctypes.c_int())
    _lib.check(_lib.lib().bk_selection_margin(engine.ctx, ctypes.byref(gap[0]),
                                              ctypes.byref(gap[1]), ctypes.byref(gap[2])))
    assert _same([gap[0].value, gap[1].value], recs[3, :2]) and gap[2].value == 1
    with pytest.raises(ValueError):  # that call had six problems
        _records(engine, 5)


def test_isolation(engine, oracle):
    """between two identical ragged calls: a single call, a bk_multikrum_batch_device
    and a collection finish -- separate queue lines, partials and descriptors;
    everyone's outputs are unchanged"""
    ns = [100, 17, 97, 20, 40, 33]
    probs, fs = _mix(ns, 257, 71)
    K = Pack(probs)
    Y = Pack([_problem(100, 257, 72)])
    U = Pack([_problem(33, 257, 73 + b) for b in range(3)])
    Z = oracle.synth(20, 200, 41, 3)
    engine.collect_begin(20, 200, Z.dtype)
    engine.collect_add([Z[r] for r in range(20)])

    def batched():
        sel = torch.full((3 * 23,), -7, dtype=torch.int64, device="cuda")
        sc = torch.full((3 * 33,), PAD, dtype=torch.float64, device="cuda")
        mean = torch.full((3 * 257,), PAD, dtype=torch.float64, device="cuda")
        engine.multikrum_batch_device_ptr(U.ptr(0), U.dt, 3, 33, 257, 257, 33 * 257, 10,
                                          sel.data_ptr(), sc.data_ptr(), mean.data_ptr())
        engine.synchronize()
        return sel.cpu().numpy(), sc.cpu().numpy(), mean.cpu().numpy(), _records(engine, 3)

    alone_single = _singles(engine, Y, [30])
    alone_batched = batched()
    alone_finish = engine.collect_finish(f=6)
    alone_rec = _record(engine)

    first = _ragged(engine, K, fs)
    _assert_bitwise(_singles(engine, Y, [30]), alone_single, "single after ragged")
    again = batched()
    assert np.array_equal(again[0], alone_batched[0])
    assert all(_same(a, b) for a, b in zip(again[1:], alone_batched[1:]))
    fin = engine.collect_finish(f=6)
    assert np.array_equal(fin[0], alone_finish[0])
    assert _same(fin[1], alone_finish[1]) and _same(fin[2], alone_finish[2])
    assert _same(_record(engine), alone_rec)
    with pytest.raises(ValueError):  # the last call is not a batched one
        _records(engine, K.B)
    second = _ragged(engine, K, fs)
    _assert_bitwise(second, first, "ragged again")
    _assert_bitwise(first, _singles(engine, K, fs), "ragged vs singles")


def test_back_to_back_on_the_stream(engine, oracle):
    """ragged calls queued on the stream with different descriptors and no
    synchronisation between them -- more of them than the staging ring has
    slots: each call's descriptors are its own when its copy runs"""
    mixes = [[100, 17, 97, 20], [20, 33, 17, 40, 48], [5, 9, 30, 3, 31], [64, 50, 100, 112],
             [17, 18], [40, 100, 33, 97, 20, 19]]
    packs = []
    for q, ns in enumerate(mixes):
        probs, fs = _mix(ns, 130, 500 + q)
        K = Pack(probs)
        packs.append((K, fs, _singles(engine, K, fs), Outs(K, fs)))
    engine.synchronize()
    for K, fs, ref, o in packs:
        o.launch(engine)
    engine.synchronize()
    last = _records(engine, packs[-1][0].B)
    for q, (K, fs, ref, o) in enumerate(packs):
        got = o.read([r[3] for r in ref] if q + 1 < len(packs) else last)
        _assert_bitwise(got, ref, ("call", q))


def test_krum_ragged(engine, oracle):
    from biscotti_amd import krum, krum_ragged
    rng = np.random.default_rng(3)
    deltas = [rng.standard_normal((n, 40)) for n in (12, 5, 28, 12, 70)]
    clips = [5, 1, 14, 6, 35]
    got = krum_ragged([[list(map(float, row)) for row in x] for x in deltas], clips, engine=engine)
    assert len(got) == 5
    for x, c, g in zip(deltas, clips, got):
        assert g.dtype == np.int64 and np.array_equal(g, krum(x, c, engine=engine))
    same = krum_ragged(deltas, 2, engine=engine)
    assert all(np.array_equal(g, krum(x, 2, engine=engine)) for x, g in zip(deltas, same))
