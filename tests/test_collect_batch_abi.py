"""bk_collect_finish_batch (include/bk.h): the symbol is exported and the
argument checks answer without a GPU -- the shape checks come before anything
that needs a context or a collection, then the null checks in the header's
order."""
import ctypes

import numpy as np
import pytest

from biscotti_amd import _lib

NAME = "bk_collect_finish_batch"


def _call(ctx, orders, batch, n, f, sel=None):
    return _lib.lib().bk_collect_finish_batch(ctx, orders, batch, n, f, sel, None, None, None)


def test_symbol_exported():
    assert NAME in _lib.SIGNATURES
    assert hasattr(_lib.lib(), NAME)


@pytest.mark.parametrize("batch,status,word", [
    (0, _lib.BK_EINVAL, "batch"),
    (-1, _lib.BK_EINVAL, "batch"),
    (_lib.BK_MAX_BATCH + 1, _lib.BK_ENOTSUP, "BK_MAX_BATCH"),
    (1, _lib.BK_EINVAL, "null context"),
    (3, _lib.BK_EINVAL, "null context"),
    (_lib.BK_MAX_BATCH, _lib.BK_EINVAL, "null context"),
])
def test_shape_checks_need_no_gpu(batch, status, word):
    """with everything else null: the shape checks answer first, then the context"""
    assert _call(None, None, batch, 10, 2) == status
    assert word in _lib.last_error(), _lib.last_error()


def test_shape_checks_come_before_the_pointers():
    """a bad batch answers whatever the pointers are"""
    orders = (ctypes.c_int64 * 20)(*range(20))
    sel = (ctypes.c_int64 * 16)()
    assert _call(None, orders, 0, 10, 2, sel) == _lib.BK_EINVAL
    assert "batch" in _lib.last_error()
    assert _call(None, orders, _lib.BK_MAX_BATCH + 1, 10, 2, sel) == _lib.BK_ENOTSUP
    assert "BK_MAX_BATCH" in _lib.last_error()
    assert _call(None, orders, 2, 10, 2, sel) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()


def test_engine_rejects_orders_that_are_not_2d():
    """Engine.collect_finish_batch's ValueError, before any GPU work: no context
    is created here"""
    from biscotti_amd.krum import Engine
    e = Engine.__new__(Engine)
    e._ctx = ctypes.c_void_p()
    for bad in (np.arange(6), np.zeros((2, 3, 4), dtype=np.int64), 5):
        with pytest.raises(ValueError, match="2-D"):
            e.collect_finish_batch(bad, 1)
    with pytest.raises(ValueError, match="integer"):
        e.collect_finish_batch(np.zeros((2, 3)), 1)
