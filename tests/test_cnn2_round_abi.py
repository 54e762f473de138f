"""The CNN2 verifier's round entries without a GPU: the prototypes in
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
    "bk_roni_cnn2_round_begin": "bk_ctx *ctx, const double *ww, int where",
    "bk_roni_cnn2_round_score_batches": "bk_ctx *ctx, bk_row_table deltas, int64_t count, int where, "
                                        "const int64_t *idx, int64_t nb, double *scores, "
                                        "int32_t *near_ties",
    "bk_roni_cnn2_round_set_band": "bk_ctx *ctx, int rows",
}
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch
P = np.zeros(8).ctypes.data


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
    new = ("bk_cnn2_round.hip", "bk_cnn2_round_api.hip")
    assert set(new) <= set(build.SOURCES)
    assert all(build.SOURCE_FLAGS[s] == build.SOURCE_FLAGS["bk_cnn2.hip"] for s in new)


# (entry, arguments) -> the refusal's words; score: (ctx, deltas, count, where, idx, nb, scores, near)
@pytest.mark.parametrize("entry,args,words", [
    ("score_batches", (None, None, 0, 9, None, 0, None, None), "null context"),
    ("score_batches", (FAKE, None, 0, 9, None, 0, None, None), "null pointer argument"),
    ("score_batches", (FAKE, P, 0, 9, None, 0, None, None), "null pointer argument"),
    ("score_batches", (FAKE, P, 0, 9, P, 0, None, None), "null pointer argument"),
    ("score_batches", (FAKE, P, 0, 9, P, 0, P, None), "count=0 < 1"),
    ("score_batches", (FAKE, P, 1, 9, P, 0, P, None), "nb >= 1"),
    ("score_batches", (FAKE, P, 1, 9, P, 1, P, None), "bad where=9"),
    ("begin", (None, P, _lib.BK_HOST), "null context"),
    ("set_band", (None, 1), "null context"),
    ("set_band", (FAKE, -1), "rows=-1 < 0"),
])
def test_stateless_refusals_in_order(entry, args, words):
    assert getattr(_lib.lib(), "bk_roni_cnn2_round_" + entry)(*args) == _lib.BK_EINVAL
    assert words in _lib.last_error()
