"""The CNN entries without a GPU: the prototypes in include/bk.h against the
bindings, the unchanged ABI version and kernel-id count, and every refusal that
needs no GPU state (they all return before the context is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "bk_eval_set_cnn": "bk_ctx *ctx, int set, const float *X, int64_t nv, int64_t ldv, "
                       "const int32_t *y, const bk_cnn_shape *shape",
    "bk_roni_cnn_set_validation": "bk_ctx *ctx, const float *Xv, int64_t nv, int64_t ldv, "
                                  "const int32_t *yv, const bk_cnn_shape *shape",
    "bk_roni_cnn_batches": "bk_ctx *ctx, const double *ww, const double *deltas, int64_t n, "
                           "int64_t ld, const int64_t *idx, int64_t nb, double *scores, "
                           "int32_t *near_ties",
}
MNIST = (28, 28, 5, 4, 16, 10)
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch


def shape(*v):
    return (ctypes.c_int32 * 6)(*v)


def test_prototypes_and_bindings():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION and len(_lib.ALL_KERNELS) == 21
    assert re.search(r"typedef struct bk_cnn_shape \{\s*int32_t h, w, k, pad, c_out, n_classes;", text)
    for name, want in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == want
        res, args = _lib.SIGNATURES[name]
        assert hasattr(L, name) and res is ctypes.c_int and len(args) == want.count(",") + 1
    assert {"bk_cnn.hip", "bk_cnn_api.hip"} <= set(build.SOURCES)


@pytest.mark.parametrize("bad", [
    (28, 28, 6, 4, 16, 10), (28, 28, 0, 0, 16, 10), (28, 28, 5, 5, 16, 10), (28, 28, 5, -1, 16, 10),
    (2, 28, 5, 1, 16, 10), (28, 2, 5, 1, 16, 10), (28, 28, 5, 4, 0, 10), (28, 28, 5, 4, 17, 10),
    (28, 28, 5, 4, 16, 1), (28, 28, 5, 4, 16, 17), (65, 28, 5, 4, 16, 10), (28, 65, 5, 4, 16, 10)])
def test_shape_limits(bad):
    L = _lib.lib()
    X, y = np.zeros((1, 65 * 65), np.float32), np.zeros(1, np.int32)
    assert L.bk_eval_set_cnn(FAKE, 0, X.ctypes.data, 1, X.shape[1], y.ctypes.data, shape(*bad)) \
        == _lib.BK_ENOTSUP
    assert L.bk_roni_cnn_set_validation(FAKE, X.ctypes.data, 1, X.shape[1], y.ctypes.data,
                                        shape(*bad)) == _lib.BK_ENOTSUP
    assert "outside" in _lib.last_error()


def test_refusals():
    L = _lib.lib()
    X, y = np.zeros((3, 784), np.float32), np.array([0, 10, 3], np.int32)
    xp, yp, sh, E = X.ctypes.data, y.ctypes.data, shape(*MNIST), _lib.BK_EINVAL
    assert L.bk_eval_set_cnn(None, 0, xp, 3, 784, yp, sh) == E
    assert L.bk_roni_cnn_set_validation(None, xp, 3, 784, yp, sh) == E
    assert L.bk_roni_cnn_batches(None, xp, xp, 1, 1, xp, 1, xp, None) == E
    assert L.bk_roni_cnn_batches(FAKE, xp, xp, 1, 1, None, 1, xp, None) == E
    for st in (4, -1):
        assert L.bk_eval_set_cnn(FAKE, st, xp, 3, 784, yp, sh) == E
    assert L.bk_eval_set_cnn(FAKE, 0, xp, 3, 784, yp, None) == E
    for nv, ldv, x_, y_ in ((0, 784, xp, yp), (3, 783, xp, yp), (3, 784, None, yp), (3, 784, xp, None)):
        assert L.bk_eval_set_cnn(FAKE, 0, x_, nv, ldv, y_, sh) == E
        assert L.bk_roni_cnn_set_validation(FAKE, x_, nv, ldv, y_, sh) == E
    assert L.bk_eval_set_cnn(FAKE, 0, xp, 3, 784, yp, sh) == E  # the label names its sample
    assert "y[1]=10" in _lib.last_error()
    ww = np.zeros(8)
    sets, out = np.zeros(1, np.intc), np.zeros(1)
    assert L.bk_eval(FAKE, ww.ctypes.data, 8, 7, sets.ctypes.data, 1, out.ctypes.data,
                     out.ctypes.data, None) == E and "bad where" in _lib.last_error()
