"""bk_collect_add_noised_finish without a GPU: the prototype in include/bk.h,
the binding in the built library with matching argument counts, the unchanged
ABI version and kernel count, and the argument checks that need no collection."""
import ctypes
import os
import re

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bk_collect_add_noised_finish"


def _proto(name):
    """the C prototype of `name` in include/bk.h, comments dropped, white space collapsed"""
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototype_and_binding():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    assert len(_lib.ALL_KERNELS) == 21
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = fh.read()
    assert re.search(r"#define\s+BK_ABI_VERSION\s+14\b", text)
    assert re.search(r"\bBK_NUM_KERNELS\s*=\s*21\b", text)
    proto = _proto(NAME)
    assert proto == (
        "bk_ctx *ctx, const double *delta, const double *const *noises, int64_t k, int where, "
        "const int64_t *order, int64_t n, int64_t f, int64_t *first_slot , int64_t *sel_idx, "
        "int64_t *m_out, double *scores, double *mean_out")
    assert hasattr(L, NAME) and NAME in _lib.SIGNATURES
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    res, args = _lib.SIGNATURES[NAME]
    assert res is i and len(args) == len(proto.split(",")) == 13
    assert args[:8] == [p, p, p, i64, i, p, i64, i64] and args[9:] == [p, p, p, p]


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
    sel = (ctypes.c_int64 * 4)()
    first = ctypes.c_int64(-7)
    _fresh_message(lambda: L.bk_collect_add_noised_finish(
        None, ctypes.addressof(row), one, 1, _lib.BK_HOST, None, 2, 1, ctypes.byref(first),
        ctypes.addressof(sel), None, None, None), _lib.BK_EINVAL, "null context")
    assert first.value == -7
    # whatever else is wrong with the call (k past the cap included), the
    # context is checked first
    _fresh_message(lambda: L.bk_collect_add_noised_finish(
        None, None, None, 65, 9, None, 0, 0, None, None, None, None, None),
        _lib.BK_EINVAL, "null context")
