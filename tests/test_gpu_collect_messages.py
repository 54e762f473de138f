"""The order checks of bk_collect_finish, bk_collect_finish_batch and
bk_collect_finish_ragged (bk_collect.hip check_order): which calls are refused,
with BK_EINVAL and exactly which bk_last_error() text -- the single finish's
without a problem number, the batched entries' with one -- and that a refused
call leaves the collection as it was.  A slot may repeat across the problems of
a batched call, never within one."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

COUNT, D, N, F = 6, 8, 4, 1
GOOD = [0, 1, 2, 3]
# the bad entry is order[2] of the problem; the batched entries carry it in problem 1
BAD = [
    ([0, 1, COUNT, 3], "order[2] = 6 is no collected slot (0..5)"),
    ([0, 1, -1, 3], "order[2] = -1 is no collected slot (0..5)"),
    ([0, 1, 1, 3], "order[2] = 1 repeats a slot"),
]
BAD3 = [  # the ragged entry's problem 1 has three rows
    ([0, 1, COUNT], "order[2] = 6 is no collected slot (0..5)"),
    ([0, 1, -1], "order[2] = -1 is no collected slot (0..5)"),
    ([5, 1, 1], "order[2] = 1 repeats a slot"),
]


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _single(engine, order, f=F):
    """-> (status, sel) of bk_collect_finish through _lib"""
    order = _i64(order)
    sel = np.full(order.size - f, -7, np.int64)
    m = ctypes.c_int64(0)
    st = _lib.lib().bk_collect_finish(engine.ctx, order.ctypes.data, order.size, f, sel.ctypes.data,
                                      ctypes.addressof(m), None, None)
    return st, sel


def _batch(engine, orders):
    orders = _i64(orders)
    B, n = orders.shape
    sel = np.full((B, n - F), -7, np.int64)
    m = ctypes.c_int64(0)
    st = _lib.lib().bk_collect_finish_batch(engine.ctx, orders.ctypes.data, B, n, F,
                                            sel.ctypes.data, ctypes.addressof(m), None, None)
    return st, sel


def _ragged(engine, orders):
    flat = _i64(np.concatenate([_i64(o) for o in orders]))
    offs = _i64(np.concatenate([[0], np.cumsum([len(o) for o in orders])]))
    fs = _i64([F] * len(orders))
    sel = np.full(int(offs[-1]) - F * len(orders), -7, np.int64)
    ms = np.zeros(len(orders), np.int64)
    st = _lib.lib().bk_collect_finish_ragged(engine.ctx, flat.ctypes.data, offs.ctypes.data,
                                             fs.ctypes.data, len(orders), sel.ctypes.data,
                                             ms.ctypes.data, None, None)
    return st, np.split(sel, np.cumsum(ms)[:-1]) if st == _lib.BK_OK else None


@pytest.fixture(scope="module")
def collected(engine):
    """one collection of 6 rows, d = 8, fp64, and the single finish's sel on GOOD"""
    X = np.random.default_rng(20261020).standard_normal((COUNT, D))
    engine.collect_begin(COUNT, D, X.dtype)
    assert engine.collect_add([X[r] for r in range(COUNT)]) == 0
    st, sel = _single(engine, GOOD)
    assert st == _lib.BK_OK, _lib.last_error()
    return sel


def _still_intact(engine, before):
    st, sel = _single(engine, GOOD)
    assert st == _lib.BK_OK, _lib.last_error()
    assert np.array_equal(sel, before), (sel, before)


@pytest.mark.parametrize("order,text", BAD)
def test_single_finish_refuses(engine, collected, order, text):
    st, _ = _single(engine, order)
    assert st == _lib.BK_EINVAL
    assert _lib.last_error() == text
    _still_intact(engine, collected)


@pytest.mark.parametrize("order,text", BAD)
def test_batch_refuses(engine, collected, order, text):
    st, _ = _batch(engine, [GOOD, order])
    assert st == _lib.BK_EINVAL
    assert _lib.last_error() == "problem 1: " + text
    _still_intact(engine, collected)


@pytest.mark.parametrize("order,text", BAD3)
def test_ragged_refuses(engine, collected, order, text):
    st, _ = _ragged(engine, [GOOD, order])
    assert st == _lib.BK_EINVAL
    assert _lib.last_error() == "problem 1: " + text
    _still_intact(engine, collected)


def test_a_slot_may_repeat_across_problems(engine, collected):
    """slots 0 and 3 (and 2) serve both problems: accepted, and each problem's
    sel is the single finish's"""
    p1, q1 = [3, 2, 5, 0], [3, 5, 0]
    ref = {tuple(o): _single(engine, o)[1] for o in (GOOD, p1, q1)}
    st, sel = _batch(engine, [GOOD, p1])
    assert st == _lib.BK_OK, _lib.last_error()
    assert np.array_equal(sel[0], ref[tuple(GOOD)]) and np.array_equal(sel[1], ref[tuple(p1)])
    st, sels = _ragged(engine, [GOOD, q1])
    assert st == _lib.BK_OK, _lib.last_error()
    assert np.array_equal(sels[0], ref[tuple(GOOD)]) and np.array_equal(sels[1], ref[tuple(q1)])
    _still_intact(engine, collected)
