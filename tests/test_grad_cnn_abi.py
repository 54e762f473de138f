"""bk_grad_set_cnn / bk_grad_cnn without a GPU: the prototypes in include/bk.h
against the bindings, the unchanged ABI version and kernel-id count, the new
sources in the build, and every refusal that needs no GPU state (they all
return before the context is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "bk_grad_set_cnn": "bk_ctx *ctx, const float *X, int64_t nn, int64_t ldx, const int32_t *y, "
                       "const bk_cnn_shape *shape",
    "bk_grad_cnn": "bk_ctx *ctx, const double *ww, int where, const int64_t *idx, int64_t count, "
                   "double max_norm, const double *noise, int precision, double *delta_out, "
                   "int64_t *q_out, double *loss_out, double *norm_out",
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
    for name, want in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == want
        res, args = _lib.SIGNATURES[name]
        assert hasattr(L, name) and res is ctypes.c_int and len(args) == want.count(",") + 1
    assert {"bk_grad_cnn.hip", "bk_grad_cnn_api.hip"} <= set(build.SOURCES)
    assert build.SOURCE_FLAGS["bk_grad_cnn.hip"] == build.SOURCE_FLAGS["bk_cnn.hip"]
    assert _lib.BK_GRAD_CNN_MAX_BATCH == 4096


@pytest.mark.parametrize("bad", [(28, 28, 6, 4, 16, 10), (28, 28, 5, 5, 16, 10), (28, 28, 5, 4, 17, 10),
                                 (28, 28, 5, 4, 16, 1), (65, 28, 5, 4, 16, 10)])
def test_shape_limits(bad):
    X, y = np.zeros((1, 65 * 65), np.float32), np.zeros(1, np.int32)
    assert _lib.lib().bk_grad_set_cnn(FAKE, X.ctypes.data, 1, X.shape[1], y.ctypes.data,
                                      shape(*bad)) == _lib.BK_ENOTSUP
    assert "outside" in _lib.last_error()


def test_set_refusals_in_order():
    L = _lib.lib()
    X, y = np.zeros((3, 784), np.float32), np.array([0, 10, 3], np.int32)
    xp, yp, sh, E = X.ctypes.data, y.ctypes.data, shape(*MNIST), _lib.BK_EINVAL
    assert L.bk_grad_set_cnn(None, xp, 3, 784, yp, sh) == E
    assert L.bk_grad_set_cnn(FAKE, xp, 3, 784, yp, None) == E
    for nn, ldx, x_, y_, word in ((0, 784, xp, yp, "nn >= 1"), (3, 783, xp, yp, "ldx=783"),
                                  (3, 784, None, yp, "null X"), (3, 784, xp, None, "null X"),
                                  (3, 784, xp, yp, "y[1]=10")):
        assert L.bk_grad_set_cnn(FAKE, x_, nn, ldx, y_, sh) == E and word in _lib.last_error()
    # the shape comes before the samples, the size before the pointers
    assert L.bk_grad_set_cnn(FAKE, None, 0, 0, None, shape(28, 28, 6, 4, 16, 10)) == _lib.BK_ENOTSUP
    assert L.bk_grad_set_cnn(FAKE, None, (1 << 31) + 1, 784, None, sh) == _lib.BK_ENOTSUP


def test_call_refusals_in_order():
    L = _lib.lib()
    w, out, q = np.zeros(8), np.zeros(8), np.zeros(8, np.int64)
    wp, op, qp, H = w.ctypes.data, out.ctypes.data, q.ctypes.data, _lib.BK_HOST

    def call(ctx=FAKE, ww=wp, where=H, max_norm=100.0, prec=4, o=op, qq=qp):
        return L.bk_grad_cnn(ctx, ww, where, None, 0, max_norm, None, prec, o, qq, None, None)

    for kw, word in ((dict(ctx=None), "null context"), (dict(ww=None), "null ww"),
                     (dict(o=None), "null delta_out"), (dict(where=7), "bad where"),
                     (dict(prec=19), "exceeds 18"), (dict(prec=-1), "without a precision"),
                     (dict(max_norm=0.0), "max_norm"), (dict(max_norm=float("nan")), "max_norm"),
                     (dict(max_norm=float("inf")), "max_norm")):
        assert call(**kw) == _lib.BK_EINVAL and word in _lib.last_error(), kw
    assert call(ww=None, max_norm=0.0) == _lib.BK_EINVAL and "null ww" in _lib.last_error()
