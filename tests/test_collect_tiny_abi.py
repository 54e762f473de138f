"""bk_set_collect_tiny and bk_collect_tiny_stats without a GPU: the prototypes in
include/bk.h, the bindings in the built library, the unchanged ABI version and
kernel count, and the argument checks that need no context."""
import ctypes
import os
import re

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proto(name):
    """the C prototype of `name` in include/bk.h, comments dropped, white space collapsed"""
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototypes_and_bindings():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    assert len(_lib.ALL_KERNELS) == 21
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = fh.read()
    assert re.search(r"#define\s+BK_ABI_VERSION\s+14\b", text)
    assert re.search(r"\bBK_NUM_KERNELS\s*=\s*21\b", text)
    assert _proto("bk_set_collect_tiny") == "bk_ctx *ctx, int on"
    assert _proto("bk_collect_tiny_stats") == "bk_ctx *ctx, int64_t out[3]"
    # the four-field stats keep their shape
    assert _proto("bk_collect_stats") == "bk_ctx *ctx, int64_t out[4]"
    i, p = ctypes.c_int, ctypes.c_void_p
    for name in ("bk_set_collect_tiny", "bk_collect_tiny_stats"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["bk_set_collect_tiny"]
    assert res is i and args == [p, i]
    res, args = _lib.SIGNATURES["bk_collect_tiny_stats"]
    assert res is i and len(args) == 2 and args[0] is p


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
    out = (ctypes.c_int64 * 3)(9, 9, 9)
    _fresh_message(lambda: L.bk_set_collect_tiny(None, 1), _lib.BK_EINVAL, "null context")
    _fresh_message(lambda: L.bk_set_collect_tiny(None, 0), _lib.BK_EINVAL, "null context")
    _fresh_message(lambda: L.bk_collect_tiny_stats(None, out), _lib.BK_EINVAL, "null context")
    assert list(out) == [9, 9, 9]
    # whatever else is wrong with the call, the context is checked first
    _fresh_message(lambda: L.bk_collect_tiny_stats(None, None), _lib.BK_EINVAL, "null context")


def test_engine_and_validator_surface():
    from biscotti_amd.krum import Engine, KRUMValidator
    assert callable(Engine.set_collect_tiny) and callable(Engine.collect_tiny_stats)
    v = KRUMValidator(collect=True, tiny=True)
    assert v._tiny and not KRUMValidator(collect=True)._tiny
    KRUMValidator(collect=True, tiny=True, noised=True)
    try:
        KRUMValidator(tiny=True)
    except ValueError as e:
        assert "collect=True" in str(e)
    else:
        raise AssertionError("tiny=True without collect=True was accepted")
