"""bk_roni_softmax_round_score_batches without a GPU: the symbol and its
prototype, the header's declaration, the refusals that need no device, and the
validator's opt-in keyword."""
import ctypes
import inspect
import os
import re

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_i, _i64, _p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
NAME = "bk_roni_softmax_round_score_batches"
# bk_ctx*, const double *const *deltas, int64_t count, int where, const int64_t *idx,
# int64_t nb, double *scores, int32_t *near_ties
PROTOTYPE = (_i, [_p, _p, _i64, _i, _p, _i64, _p, _p])


def test_symbol_and_prototype():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert _lib.SIGNATURES[NAME] == PROTOTYPE
    assert L.bk_abi_version() == 14  # added without a change of the ABI version
    # no kernel id of its own: the launches are timed as the softmax round's
    assert len(_lib.ALL_KERNELS) == 21 and L.bk_kernel_name(21) == b"?"


def test_header_declares_the_documented_prototype():
    src = open(os.path.join(REPO, "include", "bk.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    decl = ("int bk_roni_softmax_round_score_batches(bk_ctx *ctx, const double *const *deltas, "
            "int64_t count, int where, const int64_t *idx, int64_t nb, double *scores, "
            "int32_t *near_ties);")
    assert decl in flat


def test_null_context_is_refused_first():
    L = _lib.lib()
    row = (ctypes.c_double * 6)()
    table = (ctypes.c_void_p * 1)(ctypes.addressof(row))
    idx = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    out = (ctypes.c_double * 1)()
    nt = (ctypes.c_int32 * 2)()
    fn = getattr(L, NAME)
    for where in (_lib.BK_HOST, _lib.BK_HOST_PINNED, _lib.BK_DEVICE):
        assert fn(None, table, 1, where, idx, 2, out, nt) == _lib.BK_EINVAL
        assert "context" in _lib.last_error()
    # whatever else is wrong with the call, too
    assert fn(None, None, 0, 9, None, 0, None, None) == _lib.BK_EINVAL
    assert fn(None, table, -1, 0, idx, -5, out, None) == _lib.BK_EINVAL
    assert "context" in _lib.last_error()


def test_validator_keyword_without_a_gpu():
    from biscotti_amd.roni import SoftmaxRONIValidator
    sig = inspect.signature(SoftmaxRONIValidator.__init__)
    assert sig.parameters["round_batches"].default is False
    assert sig.parameters["batch_size"].default == 10
    assert inspect.signature(SoftmaxRONIValidator.score_round).parameters["idx"].default is None
