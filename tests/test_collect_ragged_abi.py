"""bk_collect_finish_ragged and bk_ragged_queue_item (include/bk.h): the symbols
are exported, the argument checks that need no GPU answer in the header's
order, and the queue map of k_collect_small_ragged -- the one thing that could
make that kernel wait for something that never comes -- is checked position by
position on the CPU, through the same function the kernel decodes with."""
import ctypes

import numpy as np
import pytest

from biscotti_amd import _lib

NAMES = ("bk_collect_finish_ragged", "bk_ragged_queue_item")


def _call(ctx, orders, offsets, fs, batch, sel=None):
    return _lib.lib().bk_collect_finish_ragged(ctx, orders, offsets, fs, batch, sel, None, None,
                                               None)


def test_symbols_exported():
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("batch,status,word", [
    (0, _lib.BK_EINVAL, "batch"),
    (-1, _lib.BK_EINVAL, "batch"),
    (_lib.BK_MAX_BATCH + 1, _lib.BK_ENOTSUP, "BK_MAX_BATCH"),
    (1, _lib.BK_EINVAL, "null context"),
    (_lib.BK_MAX_BATCH, _lib.BK_EINVAL, "null context"),
])
def test_shape_checks_need_no_gpu(batch, status, word):
    """with everything else null: the shape checks answer first, then the context"""
    assert _call(None, None, None, None, batch) == status
    assert word in _lib.last_error(), _lib.last_error()


def test_checks_in_the_headers_order():
    """a bad batch answers whatever the pointers are; then the null context; then
    the null pointers, each by name, in the header's order (a context that is
    never dereferenced: every check here comes before the first use of it)"""
    orders = (ctypes.c_int64 * 20)(*range(20))
    offsets = (ctypes.c_int64 * 3)(0, 10, 20)
    fs = (ctypes.c_int64 * 2)(2, 3)
    sel = (ctypes.c_int64 * 15)()
    assert _call(None, orders, offsets, fs, 0, sel) == _lib.BK_EINVAL
    assert "batch" in _lib.last_error()
    assert _call(None, orders, offsets, fs, _lib.BK_MAX_BATCH + 1, sel) == _lib.BK_ENOTSUP
    assert "BK_MAX_BATCH" in _lib.last_error()
    assert _call(None, orders, offsets, fs, 2, sel) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()
    block = ctypes.create_string_buffer(1 << 16)  # zeroed; outlives the calls below
    fake = ctypes.c_void_p(ctypes.addressof(block))
    for args, word in (((None, offsets, fs, 2, sel), "null orders"),
                       ((None, None, None, 2, None), "null orders"),
                       ((orders, None, fs, 2, sel), "null offsets"),
                       ((orders, None, None, 2, None), "null offsets"),
                       ((orders, offsets, None, 2, sel), "null fs"),
                       ((orders, offsets, None, 2, None), "null fs"),
                       ((orders, offsets, fs, 2, None), "null sel_idx")):
        assert _call(fake, *args) == _lib.BK_EINVAL
        assert word in _lib.last_error(), (word, _lib.last_error())


def test_engine_value_errors_need_no_context():
    """Engine.collect_finish_ragged's ValueErrors, before any GPU work: no
    context is created here"""
    from biscotti_amd.krum import Engine
    e = Engine.__new__(Engine)
    e._ctx = ctypes.c_void_p()
    with pytest.raises(ValueError, match="at least one"):
        e.collect_finish_ragged([], 1)
    for bad in ([np.zeros((2, 3), dtype=np.int64)], [np.arange(4), np.int64(5)], np.arange(6)):
        with pytest.raises(ValueError, match="1-D"):
            e.collect_finish_ragged(bad, 1)
    with pytest.raises(ValueError, match="integer"):
        e.collect_finish_ragged([np.arange(4), np.zeros(3)], 1)
    with pytest.raises(ValueError, match="one f per problem"):
        e.collect_finish_ragged([np.arange(4), np.arange(3)], [1, 1, 1])
    with pytest.raises(ValueError, match="without collect_begin"):
        e.collect_finish_ragged([np.arange(4), np.arange(3)], [1, 1])


# ---- the queue map ------------------------------------------------------------

def _decode_all(n, C):
    """every queue position of the W = len(n) problems -> (p, it), and the
    positions just outside the queue"""
    L = _lib.lib()
    n = np.ascontiguousarray(n, dtype=np.int32)
    W = len(n)
    total = int(n.sum()) + W * C
    p, it = ctypes.c_int(-7), ctypes.c_int(-7)
    for outside in (-1, total, total + 1):
        assert L.bk_ragged_queue_item(n.ctypes.data, W, C, outside, ctypes.byref(p),
                                      ctypes.byref(it)) == _lib.BK_EINVAL, outside
        assert "outside the queue" in _lib.last_error()
    out = np.empty((total, 2), dtype=np.int64)
    for item in range(total):
        assert L.bk_ragged_queue_item(n.ctypes.data, W, C, item, ctypes.byref(p),
                                      ctypes.byref(it)) == _lib.BK_OK, item
        out[item] = p.value, it.value
    return out


def _check_map(n, C):
    n = np.asarray(n, dtype=np.int64)
    W = len(n)
    q = _decode_all(n, C)
    p, it = q[:, 0], q[:, 1]
    assert p.min() >= 0 and p.max() < W and it.min() >= 0
    assert (it < n[p] + C).all()
    # each (p, S i), i < n_p, and each (p, M c), c < C, exactly once: as many
    # positions as pairs, every pair in range, and no pair twice
    key = p * 1024 + it
    assert len(np.unique(key)) == len(key) == int(n.sum()) + W * C
    pos = np.arange(len(q))
    is_s = it < n[p]
    for b in range(W):
        s_pos, m_pos = pos[(p == b) & is_s], pos[(p == b) & ~is_s]
        assert len(s_pos) == n[b] and len(m_pos) == C
        # every S item of b precedes every M item of b (M_b waits for S items
        # EARLIER in the queue), in item order
        assert s_pos.max() < m_pos.min(), b
        assert np.array_equal(it[s_pos], np.arange(n[b])) and np.array_equal(it[m_pos], n[b] + np.arange(C))
        # M_b sits behind S_{b+1}: the lag-one pipeline
        if b + 1 < W:
            assert pos[(p == b + 1) & is_s].max() < m_pos.min(), b
            # ... and ahead of S_{b+2}: the queue never runs further ahead
            if b + 2 < W:
                assert m_pos.max() < pos[(p == b + 2) & is_s].min(), b
    # the leading run, held by blockIdx: S_0 then S_1, in item order
    lead = int(n[0] + (n[1] if W > 1 else 0))
    want = [(0, i) for i in range(n[0])] + ([(1, i) for i in range(n[1])] if W > 1 else [])
    assert [tuple(r) for r in q[:lead]] == want


SIZES = (1, 2, 15, 16, 17, 128)


@pytest.mark.parametrize("C", [1, 2, 123])
@pytest.mark.parametrize("W", [1, 2, 3, 7])
def test_queue_map(W, C):
    """n from {1, 2, 15, 16, 17, 128}: every W-tuple for W <= 3, and for W = 7
    every rotation of the sizes (each size at each place) plus seeded draws"""
    import itertools
    if W <= 3:
        cases = list(itertools.product(SIZES, repeat=W))
    else:
        ring = list(SIZES) + [128]
        cases = [ring[r:] + ring[:r] for r in range(W)]
        rng = np.random.default_rng(100 * W + C)
        cases += [list(rng.choice(SIZES, size=W)) for _ in range(6)]
    for n in cases:
        _check_map(n, C)


def test_queue_map_1024_problems():
    """the largest launch: W = 1,024 (an 11-step search), seeded sizes 1..128"""
    rng = np.random.default_rng(1024)
    n = rng.integers(1, 129, size=1024)
    n[:6] = SIZES
    _check_map(n, 2)


def test_queue_item_rejects_bad_shapes():
    L = _lib.lib()
    p, it = ctypes.c_int(), ctypes.c_int()
    n = np.array([3, 4], dtype=np.int32)
    bad = np.array([3, 129], dtype=np.int32)
    for args in ((None, 2, 1, 0), (n.ctypes.data, 0, 1, 0), (n.ctypes.data, 1025, 1, 0),
                 (n.ctypes.data, 2, 0, 0), (bad.ctypes.data, 2, 1, 0)):
        assert L.bk_ragged_queue_item(*args, ctypes.byref(p), ctypes.byref(it)) == _lib.BK_EINVAL
