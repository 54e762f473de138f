"""The bk_block_* family without a GPU: the prototypes in include/bk.h, the
bindings in the built library, the unchanged ABI version and kernel count, and
every argument check that needs no block (they need no context's GPU either)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_block_begin": "bk_ctx *ctx, int dtype, int64_t d, const double *global_w, int where, "
                      "int precision",
    "bk_block_add": "bk_ctx *ctx, const void *const *rows, const uint8_t *accepted, int64_t count, "
                    "int where, int64_t *first_slot",
    "bk_block_count": "bk_ctx *ctx, int64_t *added, int64_t *accepted",
    "bk_block_finish": "bk_ctx *ctx, double *global_out, int64_t *qsum_out, double *qsum_float_out",
    "bk_block_add_finish": "bk_ctx *ctx, const void *row, int accepted, int where, "
                           "int64_t *first_slot, double *global_out, int64_t *qsum_out, "
                           "double *qsum_float_out",
    "bk_block_stats": "bk_ctx *ctx, int64_t out[4]",
}


def _proto(name):
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototypes_and_bindings():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    assert len(_lib.ALL_KERNELS) == 21
    for name, want in PROTOS.items():
        assert _proto(name) == want
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == want.count(",") + 1 and args[0] is ctypes.c_void_p


def _fresh_message(call, word):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == _lib.BK_EINVAL
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, msg


def test_null_context_is_einval():
    L = _lib.lib()
    g = np.zeros(4)
    rows = (ctypes.c_void_p * 1)(g.ctypes.data)
    cnt = ctypes.c_int64(7)
    out = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    gp = g.ctypes.data
    for call in (lambda: L.bk_block_begin(None, _lib.BK_F64, 4, gp, _lib.BK_HOST, -1),
                 lambda: L.bk_block_add(None, rows, None, 1, _lib.BK_HOST, None),
                 lambda: L.bk_block_count(None, ctypes.byref(cnt), ctypes.byref(cnt)),
                 lambda: L.bk_block_finish(None, gp, None, None),
                 lambda: L.bk_block_add_finish(None, gp, 1, _lib.BK_HOST, None, gp, None, None),
                 lambda: L.bk_block_stats(None, out),
                 # whatever else is wrong with the call, the context is checked first
                 lambda: L.bk_block_begin(None, 7, 0, None, 9, 99),
                 lambda: L.bk_block_stats(None, None)):
        _fresh_message(call, "null context")
    assert cnt.value == 7 and list(out) == [9, 9, 9, 9]


# The checks behind the context: the entries never dereference the handle before
# they have passed, so a context that was never created stands in for one.  It
# is only ever refused.
class _Ctx(ctypes.Structure):
    _fields_ = [("pad", ctypes.c_char * 1)]


@pytest.mark.parametrize("prec", [19, -2, 100, -100])
def test_begin_refuses_precision(prec):
    L = _lib.lib()
    g = np.zeros(4)
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    _fresh_message(lambda: L.bk_block_begin(fake, _lib.BK_F64, 4, g.ctypes.data, _lib.BK_HOST, prec),
                   "precision=%d" % prec)


def test_bad_arguments_need_no_block():
    L = _lib.lib()
    g = np.zeros(4)
    gp = g.ctypes.data
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    rows = (ctypes.c_void_p * 1)(gp)
    cnt = ctypes.c_int64(0)
    out4 = (ctypes.c_int64 * 4)()
    H = _lib.BK_HOST
    cases = [
        (lambda: L.bk_block_begin(fake, 2, 4, gp, H, -1), "dtype"),
        (lambda: L.bk_block_begin(fake, -1, 4, gp, H, -1), "dtype"),
        (lambda: L.bk_block_begin(fake, _lib.BK_F64, 0, gp, H, -1), "d=0"),
        (lambda: L.bk_block_begin(fake, _lib.BK_F32, -5, gp, H, 4), "d=-5"),
        (lambda: L.bk_block_begin(fake, _lib.BK_F64, 4, None, H, -1), "null global_w"),
        (lambda: L.bk_block_begin(fake, _lib.BK_F64, 4, gp, 3, -1), "where=3"),
        (lambda: L.bk_block_begin(fake, _lib.BK_F64, 4, gp, -1, -1), "where=-1"),
        (lambda: L.bk_block_add(fake, None, None, 1, H, None), "null rows"),
        (lambda: L.bk_block_add(fake, rows, None, 0, H, None), "count=0"),
        (lambda: L.bk_block_add(fake, rows, None, -3, H, None), "count=-3"),
        (lambda: L.bk_block_add(fake, rows, None, 1, 5, None), "where=5"),
        (lambda: L.bk_block_count(fake, None, ctypes.byref(cnt)), "null"),
        (lambda: L.bk_block_count(fake, ctypes.byref(cnt), None), "null"),
        (lambda: L.bk_block_finish(fake, None, None, None), "null global_out"),
        (lambda: L.bk_block_add_finish(fake, None, 1, H, None, gp, None, None), "null row"),
        (lambda: L.bk_block_add_finish(fake, gp, 1, 4, None, gp, None, None), "where=4"),
        (lambda: L.bk_block_add_finish(fake, gp, 1, H, None, None, None, None), "null global_out"),
        (lambda: L.bk_block_stats(fake, None), "null out"),
    ]
    for call, word in cases:
        _fresh_message(call, word)
    assert list(out4) == [0, 0, 0, 0]


def test_engine_and_collector_surface():
    from biscotti_amd import aggregate
    from biscotti_amd.krum import Engine
    for name in ("block_begin", "block_add", "block_count", "block_finish", "block_add_finish",
                 "block_stats", "block_begin_ptr", "block_add_ptr", "block_finish_ptr",
                 "block_add_finish_ptr"):
        assert callable(getattr(Engine, name)), name
    assert "BlockCollector" in aggregate.__all__
    for name in ("add_update", "create_block", "quantized_sum", "flush"):
        assert callable(getattr(aggregate.BlockCollector, name)), name
    assert "create_block" in aggregate.__all__
