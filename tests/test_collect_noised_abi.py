"""bk_collect_add_noised and bk_collect_read_rows without a GPU: the symbols and
their signatures, the unchanged ABI version, and the argument checks that need
no context."""
import ctypes
import os
import re

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proto(name):
    """the C prototype of `name` in include/bk.h, white space collapsed"""
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = fh.read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_symbols_and_signatures():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    for name in ("bk_collect_add_noised", "bk_collect_read_rows"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    res, args = _lib.SIGNATURES["bk_collect_add_noised"]
    assert res is i and args[:6] == [p, p, p, i64, i64, i] and len(args) == 7
    res, args = _lib.SIGNATURES["bk_collect_read_rows"]
    assert res is i and args == [p, p, i64, p]
    assert _proto("bk_collect_add_noised") == (
        "bk_ctx *ctx, const double *const *deltas, const double *const *noises, int64_t k, "
        "int64_t count, int where, int64_t *first_slot")
    assert _proto("bk_collect_read_rows") == (
        "bk_ctx *ctx, const int64_t *slots, int64_t count, double *const *out_rows")
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = fh.read()
    assert re.search(r"#define\s+BK_COLLECT_NOISE_MAX_K\s+64\b", text)
    assert re.search(r"#define\s+BK_ABI_VERSION\s+14\b", text)
    assert _lib.BK_COLLECT_NOISE_MAX_K == 64


def _fresh_message(call, status, word):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == status
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, msg


def test_null_context_is_einval():
    L = _lib.lib()
    row = (ctypes.c_double * 4)()
    one = (ctypes.c_void_p * 1)(ctypes.addressof(row))
    first = ctypes.c_int64(-7)
    slot = (ctypes.c_int64 * 1)(0)
    _fresh_message(lambda: L.bk_collect_add_noised(None, one, one, 1, 1, _lib.BK_HOST,
                                                   ctypes.byref(first)),
                   _lib.BK_EINVAL, "null context")
    assert first.value == -7
    # whatever else is wrong with the call, the context is checked first
    _fresh_message(lambda: L.bk_collect_add_noised(None, None, None, 65, 0, 9, None),
                   _lib.BK_EINVAL, "null context")
    _fresh_message(lambda: L.bk_collect_read_rows(None, slot, 1, one), _lib.BK_EINVAL,
                   "null context")
    _fresh_message(lambda: L.bk_collect_read_rows(None, None, 0, None), _lib.BK_EINVAL,
                   "null context")
