"""The RONI round entries (bk_roni_round_* / bk_roni_softmax_round_*) without a
GPU: the symbols and prototypes, the kernel ids of their launches, and the
argument checks that need no device."""
import ctypes
import os
import re

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_i, _i64, _p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
PROTOTYPES = {
    # bk_ctx*, const double *ww, int64_t d, int where
    "bk_roni_round_begin": (_i, [_p, _p, _i64, _i]),
    # bk_ctx*, const double *const *deltas, int64_t count, int where, double *scores
    "bk_roni_round_score": (_i, [_p, _p, _i64, _i, _p]),
    # bk_ctx*, const double *ww, int where
    "bk_roni_softmax_round_begin": (_i, [_p, _p, _i]),
    # bk_ctx*, deltas, count, where, double *scores, int32_t *near_ties
    "bk_roni_softmax_round_score": (_i, [_p, _p, _i64, _i, _p, _p]),
}


def test_symbols_and_prototypes():
    L = _lib.lib()
    for name, proto in PROTOTYPES.items():
        assert hasattr(L, name), name
        assert _lib.SIGNATURES[name] == proto, name
    assert L.bk_abi_version() == 14  # added without a change of the ABI version


def test_header_declares_the_documented_prototypes():
    src = open(os.path.join(REPO, "include", "bk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    for decl in (
        "int bk_roni_round_begin(bk_ctx *ctx, const double *ww, int64_t d, int where);",
        "int bk_roni_round_score(bk_ctx *ctx, const double *const *deltas, int64_t count, "
        "int where, double *scores);",
        "int bk_roni_softmax_round_begin(bk_ctx *ctx, const double *ww, int where);",
        "int bk_roni_softmax_round_score(bk_ctx *ctx, const double *const *deltas, "
        "int64_t count, int where, double *scores, int32_t *near_ties);",
    ):
        assert decl in flat, decl
    assert re.search(r"#define BK_RONI_ROUND_G 8\b", src)
    assert _lib.BK_RONI_ROUND_G == 8


def test_kernel_ids():
    L = _lib.lib()
    assert _lib.ROUND_KERNELS == ["k_roni_round", "k_roni_round_sm"]
    assert _lib.K["k_roni_round"] == 19 and _lib.K["k_roni_round_sm"] == 20
    for i, name in enumerate(_lib.ALL_KERNELS):
        assert L.bk_kernel_name(i) == name.encode()
    assert L.bk_kernel_name(len(_lib.ALL_KERNELS)) == b"?"
    src = open(os.path.join(REPO, "include", "bk.h")).read()
    assert re.search(r"BK_K_RONI_ROUND = 19\b", src) and re.search(r"BK_K_RONI_ROUND_SM = 20\b", src)
    # bk_timing_read knows them (its context check comes first)
    assert L.bk_timing_read(None, 20, None, None) == _lib.BK_EINVAL


def test_null_context_is_refused():
    L = _lib.lib()
    ww = (ctypes.c_double * 4)()
    row = (ctypes.c_double * 4)()
    table = (ctypes.c_void_p * 1)(ctypes.addressof(row))
    out = (ctypes.c_double * 1)()
    nt = (ctypes.c_int32 * 2)()
    for where in (_lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE):
        assert L.bk_roni_round_begin(None, ww, 4, where) == _lib.BK_EINVAL
        assert "context" in _lib.last_error()
        assert L.bk_roni_round_score(None, table, 1, where, out) == _lib.BK_EINVAL
        assert L.bk_roni_softmax_round_begin(None, ww, where) == _lib.BK_EINVAL
        assert L.bk_roni_softmax_round_score(None, table, 1, where, out, nt) == _lib.BK_EINVAL
        assert "context" in _lib.last_error()
    assert L.bk_roni_round_score(None, None, 0, 9, None) == _lib.BK_EINVAL
    assert L.bk_roni_softmax_round_score(None, None, -1, 9, None, None) == _lib.BK_EINVAL


def test_validator_api_without_a_gpu():
    """The Python surface exists and refuses a mini-batch validator's rounds in
    its signature (no device is touched here)."""
    import inspect
    from biscotti_amd.roni import RONIValidator, SoftmaxRONIValidator
    for cls in (RONIValidator, SoftmaxRONIValidator):
        assert callable(cls.begin_round) and callable(cls.score_round)
        sig = inspect.signature(cls.verify_update)
        assert sig.parameters["round"].default is False
