"""The CNN verifier's round entries without a GPU: the prototypes in
include/bk.h against the bindings, the unchanged ABI version and kernel-id
count, the sources in the build, and every refusal that needs no GPU state, in
the documented order (each case also breaks everything checked after it)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "bk_roni_cnn_round_begin": "bk_ctx *ctx, const double *ww, int where",
    "bk_roni_cnn_round_score_batches": "bk_ctx *ctx, const double *const *deltas, int64_t count, "
                                       "int where, const int64_t *idx, int64_t nb, double *scores, "
                                       "int32_t *near_ties",
}
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch
BUF = np.zeros(8)
P = BUF.ctypes.data


def test_prototypes_and_bindings():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION and len(_lib.ALL_KERNELS) == 21
    for name, want in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == want
        res, args = _lib.SIGNATURES[name]
        assert hasattr(L, name) and res is ctypes.c_int and len(args) == want.count(",") + 1
    assert {"bk_cnn_round.hip", "bk_cnn_round_api.hip"} <= set(build.SOURCES)
    assert all(build.SOURCE_FLAGS[s] == build.NO_PACKED_FP32
               for s in ("bk_cnn_round.hip", "bk_cnn_round_api.hip"))


# (ctx, deltas, count, where, idx, nb, scores) -> the refusal's words
@pytest.mark.parametrize("args,words", [
    ((None, None, 0, 9, None, 0, None), "null context"),
    ((FAKE, None, 0, 9, None, 0, None), "null pointer argument"),
    ((FAKE, P, 0, 9, None, 0, None), "null pointer argument"),
    ((FAKE, P, 0, 9, P, 0, None), "null pointer argument"),
    ((FAKE, P, 0, 9, P, 0, P), "count=0 < 1"),
    ((FAKE, P, 1, 9, P, 0, P), "nb >= 1"),
    ((FAKE, P, 1, 9, P, 1, P), "bad where=9"),
])
def test_score_refusals_in_order(args, words):
    ctx, deltas, count, where, idx, nb, scores = args
    L = _lib.lib()
    assert L.bk_roni_cnn_round_score_batches(ctx, deltas, count, where, idx, nb, scores,
                                             None) == _lib.BK_EINVAL
    assert words in _lib.last_error()


def test_begin_refuses_a_null_context():
    assert _lib.lib().bk_roni_cnn_round_begin(None, P, _lib.BK_HOST) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()
