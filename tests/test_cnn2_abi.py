"""The two-layer CNN's entries without a GPU: the prototypes in include/bk.h
against the bindings, the unchanged ABI version and kernel-id count, and every
refusal that needs no GPU state (they all return before the context is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "bk_eval_set_cnn2": "bk_ctx *ctx, int set, const float *X, int64_t nv, int64_t ldv, "
                        "const int32_t *y, const bk_cnn2_shape *shape",
    "bk_roni_cnn2_set_validation": "bk_ctx *ctx, const float *Xv, int64_t nv, int64_t ldv, "
                                   "const int32_t *yv, const bk_cnn2_shape *shape",
    "bk_roni_cnn2_batches": "bk_ctx *ctx, const double *ww, const double *deltas, int64_t n, "
                            "int64_t ld, const int64_t *idx, int64_t nb, double *scores, "
                            "int32_t *near_ties",
}
LFW = (3, 62, 47, 3, 1, 18, 36, 2)
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch


def shape(*v):
    return (ctypes.c_int32 * 8)(*v)


def test_prototypes_and_bindings():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION and len(_lib.ALL_KERNELS) == 21
    assert re.search(r"typedef struct bk_cnn2_shape \{\s*int32_t c_in, h, w, k, pad, c1, c2, n_classes;", text)
    for name, want in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == want
        res, args = _lib.SIGNATURES[name]
        assert hasattr(L, name) and res is ctypes.c_int and len(args) == want.count(",") + 1
    assert {"bk_cnn2.hip", "bk_cnn2_api.hip"} <= set(build.SOURCES)


@pytest.mark.parametrize("bad", [
    (0, 62, 47, 3, 1, 18, 36, 2), (4, 62, 47, 3, 1, 18, 36, 2), (3, 1, 47, 3, 1, 18, 36, 2),
    (3, 62, 1, 3, 1, 18, 36, 2), (3, 65, 47, 3, 1, 18, 36, 2), (3, 62, 65, 3, 1, 18, 36, 2),
    (3, 62, 47, 0, 0, 18, 36, 2), (3, 62, 47, 4, 1, 18, 36, 2), (3, 62, 47, 3, 3, 18, 36, 2),
    (3, 62, 47, 3, -1, 18, 36, 2), (3, 62, 47, 3, 1, 0, 36, 2), (3, 62, 47, 3, 1, 33, 36, 2),
    (3, 62, 47, 3, 1, 18, 0, 2), (3, 62, 47, 3, 1, 18, 49, 2), (3, 62, 47, 3, 1, 18, 36, 1),
    (3, 62, 47, 3, 1, 18, 36, 17),
    (3, 2, 47, 3, 0, 18, 36, 2),    # the first pooled map is empty
    (3, 62, 5, 3, 0, 18, 36, 2),    # the second
    (3, 64, 64, 3, 1, 32, 36, 2)])  # the maps exceed the LDS budget
def test_shape_limits(bad):
    L = _lib.lib()
    X, y = np.zeros((1, 3 * 65 * 65), np.float32), np.zeros(1, np.int32)
    assert L.bk_eval_set_cnn2(FAKE, 0, X.ctypes.data, 1, X.shape[1], y.ctypes.data, shape(*bad)) \
        == _lib.BK_ENOTSUP
    assert L.bk_roni_cnn2_set_validation(FAKE, X.ctypes.data, 1, X.shape[1], y.ctypes.data,
                                         shape(*bad)) == _lib.BK_ENOTSUP
    assert "outside" in _lib.last_error()


def test_refusals():
    L = _lib.lib()
    din = 3 * 62 * 47
    X, y = np.zeros((3, din), np.float32), np.array([0, 2, 1], np.int32)
    xp, yp, sh, E = X.ctypes.data, y.ctypes.data, shape(*LFW), _lib.BK_EINVAL
    assert L.bk_eval_set_cnn2(None, 0, xp, 3, din, yp, sh) == E
    assert L.bk_roni_cnn2_set_validation(None, xp, 3, din, yp, sh) == E
    assert L.bk_roni_cnn2_batches(None, xp, xp, 1, 1, xp, 1, xp, None) == E
    assert L.bk_roni_cnn2_batches(FAKE, xp, xp, 1, 1, None, 1, xp, None) == E
    for st in (4, -1):
        assert L.bk_eval_set_cnn2(FAKE, st, xp, 3, din, yp, sh) == E
    assert L.bk_eval_set_cnn2(FAKE, 0, xp, 3, din, yp, None) == E
    for nv, ldv, x_, y_ in ((0, din, xp, yp), (3, din - 1, xp, yp), (3, din, None, yp), (3, din, xp, None)):
        assert L.bk_eval_set_cnn2(FAKE, 0, x_, nv, ldv, y_, sh) == E
        assert L.bk_roni_cnn2_set_validation(FAKE, x_, nv, ldv, y_, sh) == E
    assert L.bk_eval_set_cnn2(FAKE, 0, xp, 3, din, yp, sh) == E  # the label names its sample
    assert "y[1]=2" in _lib.last_error()
