"""The incremental entries (bk_collect_*) without a GPU: a NULL context is
BK_EINVAL with a message, from every one of them."""
import ctypes

import pytest

from biscotti_amd import _lib


def _calls():
    L = _lib.lib()
    row = (ctypes.c_double * 4)()
    rows = (ctypes.c_void_p * 1)(ctypes.addressof(row))
    first, cnt, mo = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    sel = (ctypes.c_int64 * 4)()
    return {
        "bk_collect_begin": lambda: L.bk_collect_begin(None, _lib.BK_F64, 4, 4),
        "bk_collect_add": lambda: L.bk_collect_add(None, rows, 1, _lib.BK_HOST,
                                                   ctypes.byref(first)),
        "bk_collect_count": lambda: L.bk_collect_count(None, ctypes.byref(cnt)),
        "bk_collect_finish": lambda: L.bk_collect_finish(None, None, 4, 1, sel,
                                                         ctypes.addressof(mo), None, None),
    }


@pytest.mark.parametrize("name", ["bk_collect_begin", "bk_collect_add", "bk_collect_count",
                                  "bk_collect_finish"])
def test_null_context_is_einval(name):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert _calls()[name]() == _lib.BK_EINVAL
    msg = _lib.last_error()
    assert msg and msg != before and "null context" in msg
