"""bk_multikrum_ragged_device, bk_multikrum_ragged and bk_ragged_batch_queue_item
(include/bk.h): the symbols are exported, the argument checks that need no GPU
answer in the header's order, and the queue map of k_small_ragged -- the one
thing that could make that kernel wait for something that never comes -- is
checked position by position on the CPU, through the same function the kernel
decodes with."""
import ctypes

import numpy as np
import pytest

from biscotti_amd import _lib

NAMES = ("bk_multikrum_ragged_device", "bk_multikrum_ragged", "bk_ragged_batch_queue_item")


def _dev(ctx, x, batch, offsets, fs, d=8, ld=8, sel=None, dtype=_lib.BK_F64):
    return _lib.lib().bk_multikrum_ragged_device(ctx, x, dtype, batch, offsets, fs, d, ld, sel,
                                                 None, None)


def _host(ctx, x, batch, offsets, fs, d=8, ld=8, sel=None, dtype=_lib.BK_F64,
          where=_lib.BK_HOST):
    return _lib.lib().bk_multikrum_ragged(ctx, x, where, dtype, batch, offsets, fs, d, ld, sel,
                                          None, None, None)


ENTRIES = pytest.mark.parametrize("call", [_dev, _host], ids=["device", "host"])


def test_symbols_exported():
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


@ENTRIES
@pytest.mark.parametrize("kw,status,word", [
    (dict(batch=1, dtype=7), _lib.BK_EINVAL, "dtype"),
    (dict(batch=0, dtype=7), _lib.BK_EINVAL, "dtype"),
    (dict(batch=0), _lib.BK_EINVAL, "batch"),
    (dict(batch=-1), _lib.BK_EINVAL, "batch"),
    (dict(batch=_lib.BK_MAX_BATCH + 1), _lib.BK_ENOTSUP, "BK_MAX_BATCH"),
    (dict(batch=0, d=0), _lib.BK_EINVAL, "batch"),
    (dict(batch=1, d=0, ld=0), _lib.BK_EINVAL, "d >= 1"),
    (dict(batch=1, d=8, ld=7), _lib.BK_EINVAL, "ld=7"),
    (dict(batch=1), _lib.BK_EINVAL, "null context"),
    (dict(batch=_lib.BK_MAX_BATCH), _lib.BK_EINVAL, "null context"),
])
def test_shape_checks_need_no_gpu(call, kw, status, word):
    """with everything else null: the dtype, then the shape checks, then the context"""
    kw = dict(kw)
    assert call(None, None, kw.pop("batch"), None, None, **kw) == status
    assert word in _lib.last_error(), _lib.last_error()


@ENTRIES
def test_checks_in_the_headers_order(call):
    """the null pointers each by name, then offsets[0], a problem without rows,
    bk_check_args per problem behind "problem b: " and, for the host entry, the
    bad `where` last (a context that is never dereferenced: every check here
    comes before the first use of it)"""
    x = (ctypes.c_double * (20 * 8))()
    offsets = (ctypes.c_int64 * 3)(0, 10, 20)
    fs = (ctypes.c_int64 * 2)(2, 3)
    sel = (ctypes.c_int64 * 15)()
    block = ctypes.create_string_buffer(1 << 16)  # zeroed; outlives the calls below
    fake = ctypes.c_void_p(ctypes.addressof(block))
    selname = "null d_sel_idx" if call is _dev else "null sel_idx"
    assert call(None, x, 2, offsets, fs, sel=sel) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()
    for args, word in (((None, 2, offsets, fs, 8, 8, sel), "null X"),
                       ((None, 2, None, None, 8, 8, None), "null X"),
                       ((x, 2, None, fs, 8, 8, sel), "null offsets"),
                       ((x, 2, None, None, 8, 8, None), "null offsets"),
                       ((x, 2, offsets, None, 8, 8, sel), "null fs"),
                       ((x, 2, offsets, None, 8, 8, None), "null fs"),
                       ((x, 2, offsets, fs, 8, 8, None), selname)):
        assert call(fake, *args) == _lib.BK_EINVAL
        assert word in _lib.last_error(), (word, _lib.last_error())
    # a bad shape answers before any of them
    assert call(fake, None, 2, None, None, 8, 7, None) == _lib.BK_EINVAL
    assert "ld=7" in _lib.last_error()
    # offsets[0] != 0 comes before a bad problem
    bad0 = (ctypes.c_int64 * 3)(1, 1, 20)
    assert call(fake, x, 2, bad0, fs, sel=sel) == _lib.BK_EINVAL
    assert "offsets[0]" in _lib.last_error()
    # a problem without rows, named, before any bk_check_args (problem 0's f is bad too)
    empty = (ctypes.c_int64 * 3)(0, 10, 10)
    badf = (ctypes.c_int64 * 2)(10, 3)
    assert call(fake, x, 2, empty, badf, sel=sel) == _lib.BK_EINVAL
    assert "problem 1: n" in _lib.last_error(), _lib.last_error()
    back = (ctypes.c_int64 * 3)(0, 10, 4)
    assert call(fake, x, 2, back, fs, sel=sel) == _lib.BK_EINVAL
    assert "problem 1: n" in _lib.last_error(), _lib.last_error()
    # bk_check_args's status and message, behind the problem
    assert _lib.lib().bk_check_args(10, 8, 10) == _lib.BK_EINVAL
    why = _lib.last_error()
    assert call(fake, x, 2, offsets, (ctypes.c_int64 * 2)(2, 10), sel=sel) == _lib.BK_EINVAL
    assert _lib.last_error() == "problem 1: " + why
    if call is _host:
        # ... which comes before the bad `where`, and the `where` before the context's use
        assert _host(fake, x, 2, offsets, badf, sel=sel, where=_lib.BK_DEVICE) == _lib.BK_EINVAL
        assert _lib.last_error().startswith("problem 0: ")
        assert _host(fake, x, 2, offsets, fs, sel=sel, where=_lib.BK_DEVICE) == _lib.BK_EINVAL
        assert "where" in _lib.last_error()


def test_engine_value_errors_need_no_context():
    """Engine.multikrum_ragged's and krum_ragged's ValueErrors, before any GPU
    work: no context is created here"""
    from biscotti_amd import krum_ragged
    from biscotti_amd.krum import Engine
    e = Engine.__new__(Engine)
    e._ctx = ctypes.c_void_p()
    with pytest.raises(ValueError, match="at least one"):
        e.multikrum_ragged([], 1)
    for bad in ([np.zeros(3)], [np.zeros((4, 3)), np.zeros((2, 2, 3))], np.zeros((4, 3))):
        with pytest.raises(ValueError, match="2-D"):
            e.multikrum_ragged(bad, 1)
    with pytest.raises(ValueError, match="share d"):
        e.multikrum_ragged([np.zeros((4, 3)), np.zeros((5, 4))], 1)
    with pytest.raises(ValueError, match="share a dtype"):
        e.multikrum_ragged([np.zeros((4, 3)), np.zeros((5, 3), dtype=np.float32)], 1)
    with pytest.raises(ValueError, match="one f per problem"):
        e.multikrum_ragged([np.zeros((4, 3)), np.zeros((5, 3))], [1, 1, 1])
    with pytest.raises(ValueError, match="one entry more"):
        e.multikrum_ragged_device_ptr(0, _lib.BK_F64, [0, 4], [1, 1], 3, 3, 0)
    # the library's own checks: the null context answers before any problem is looked at
    with pytest.raises(ValueError, match="null context"):
        e.multikrum_ragged([np.zeros((4, 3)), np.zeros((5, 3))], [1, 9])
    deltas = [np.zeros((5, 3)), np.zeros((4, 3))]
    for clips in (0, [1, 4], [5, 1]):
        with pytest.raises(ValueError, match="out of bounds"):
            krum_ragged(deltas, clips)
    with pytest.raises(ValueError, match="one clip per batch"):
        krum_ragged(deltas, [1, 1, 1])
    with pytest.raises(ValueError, match="at least one"):
        krum_ragged([], 1)


# ---- the queue map ------------------------------------------------------------

def _decode_all(n, NGI, C):
    """every queue position of the W = len(n) problems -> (p, it); the position
    `total` and its neighbours outside the queue are BK_EINVAL"""
    L = _lib.lib()
    n = np.ascontiguousarray(n, dtype=np.int32)
    W = len(n)
    total = int(n.sum()) + W * (NGI + C)
    p, it = ctypes.c_int(-7), ctypes.c_int(-7)
    for outside in (-1, total, total + 1):
        assert L.bk_ragged_batch_queue_item(n.ctypes.data, W, NGI, C, outside, ctypes.byref(p),
                                            ctypes.byref(it)) == _lib.BK_EINVAL, outside
        assert "outside the queue" in _lib.last_error()
    out = np.empty((total, 2), dtype=np.int64)
    for item in range(total):
        assert L.bk_ragged_batch_queue_item(n.ctypes.data, W, NGI, C, item, ctypes.byref(p),
                                            ctypes.byref(it)) == _lib.BK_OK, item
        out[item] = p.value, it.value
    return out


def _check_map(n, NGI, C):
    n = np.asarray(n, dtype=np.int64)
    W = len(n)
    q = _decode_all(n, NGI, C)
    total = len(q)
    p, it = q[:, 0], q[:, 1]
    assert p.min() >= 0 and p.max() < W and it.min() >= 0
    assert (it < NGI + n[p] + C).all()
    # every (p, item) exactly once: as many positions as pairs, every pair in
    # range, and no pair twice
    key = p * 4096 + it
    assert len(np.unique(key)) == len(key) == int(n.sum()) + W * (NGI + C)
    pos = np.arange(total)
    is_g = it < NGI
    is_s = ~is_g & (it < NGI + n[p])
    is_m = ~is_g & ~is_s
    for b in range(W):
        g_pos, s_pos, m_pos = (pos[(p == b) & k] for k in (is_g, is_s, is_m))
        assert len(g_pos) == NGI and len(s_pos) == n[b] and len(m_pos) == C
        # every S item of b comes after all NGI G items of b, every M item of b
        # after all n_b S items of b (each waits for items EARLIER in the queue)
        assert g_pos.max() < s_pos.min(), b
        assert s_pos.max() < m_pos.min(), b
        # ... each kind in item order
        assert np.array_equal(it[g_pos], np.arange(NGI))
        assert np.array_equal(it[s_pos], NGI + np.arange(n[b]))
        assert np.array_equal(it[m_pos], NGI + n[b] + np.arange(C))
        # the lag-one pipeline: S_b sits behind G_{b+1} and ahead of G_{b+2}
        if b + 1 < W:
            assert pos[(p == b + 1) & is_g].max() < s_pos.min(), b
            if b + 2 < W:
                assert m_pos.max() < pos[(p == b + 2) & is_g].min(), b
    # the leading run, held by blockIdx and waiting for nothing: only G items.
    # (2 NGI of them when there are two problems; one problem has NGI in all)
    lead = min((2 if W > 1 else 1) * NGI, total)
    assert is_g[:lead].all()
    want = [(0, i) for i in range(NGI)] + ([(1, i) for i in range(NGI)] if W > 1 else [])
    assert [tuple(r) for r in q[:lead]] == want


@pytest.mark.parametrize("n,NGI,C", [
    ([17], 4, 1),
    ([17, 32], 8, 3),
    ([33, 48, 40], 12, 1),
    ([2, 16, 9, 1, 16], 4, 2),
], ids=["one", "two", "three", "five"])
def test_queue_map(n, NGI, C):
    _check_map(n, NGI, C)


def test_queue_map_1024_problems():
    """the largest launch: W = 1,024 (an 11-step search) of config B's item
    counts (d = 7,850: 248 G items, 123 M items), seeded n in 113..128"""
    rng = np.random.default_rng(1024)
    _check_map(rng.integers(113, 129, size=1024), 248, 123)


def test_queue_item_rejects_bad_shapes():
    L = _lib.lib()
    p, it = ctypes.c_int(), ctypes.c_int()
    n = np.array([3, 4], dtype=np.int32)
    bad = np.array([3, 129], dtype=np.int32)
    for args in ((None, 2, 4, 1, 0), (n.ctypes.data, 0, 4, 1, 0), (n.ctypes.data, 1025, 4, 1, 0),
                 (n.ctypes.data, 2, 0, 1, 0), (n.ctypes.data, 2, 4, 0, 0),
                 (bad.ctypes.data, 2, 4, 1, 0)):
        assert L.bk_ragged_batch_queue_item(*args, ctypes.byref(p),
                                            ctypes.byref(it)) == _lib.BK_EINVAL
