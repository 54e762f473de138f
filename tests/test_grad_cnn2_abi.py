"""bk_grad_set_cnn2 / bk_grad_cnn2 without a GPU: prototypes against bindings, ABI 14, 21 kernels, the new
sources, the batch cap, the shape limits and every refusal that returns before the context is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build
from test_grad_cnn_abi import PROTOS as ONE, REPO

PROTOS = {"bk_grad_set_cnn2": ONE["bk_grad_set_cnn"].replace("bk_cnn_shape", "bk_cnn2_shape"),
          "bk_grad_cnn2": ONE["bk_grad_cnn"]}  # the one-layer entries' argument lists
LFW, DIN = (3, 62, 47, 3, 1, 18, 36, 2), 3 * 62 * 47
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch


shape = lambda *v: (ctypes.c_int32 * 8)(*v)  # noqa: E731


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
    assert {"bk_grad_cnn2.hip", "bk_grad_cnn2_api.hip"} <= set(build.SOURCES)
    assert all(build.SOURCE_FLAGS[s] == build.SOURCE_FLAGS["bk_cnn2.hip"] for s in ("bk_grad_cnn2.hip", "bk_grad_cnn2_api.hip"))
    assert _lib.BK_GRAD_CNN2_MAX_BATCH == 1024


# outside bk_cnn2_shape's limits; then inside them, but the step's forward needs 135,252 bytes of LDS
@pytest.mark.parametrize("bad,word", [((4, 62, 47, 3, 1, 18, 36, 2), "outside"), ((3, 62, 47, 4, 1, 18, 36, 2), "outside"),
                                      ((3, 62, 47, 3, 3, 18, 36, 2), "outside"), ((3, 62, 47, 3, 1, 33, 36, 2), "outside"),
                                      ((3, 62, 47, 3, 1, 18, 36, 1), "outside"), ((3, 64, 64, 3, 1, 13, 48, 2), "LDS")])
def test_shape_limits(bad, word):
    L = _lib.lib()
    assert L.bk_grad_set_cnn2(FAKE, None, 0, 0, None, shape(*bad)) == _lib.BK_ENOTSUP and word in _lib.last_error()
    for ok in (LFW, (3, 64, 64, 3, 1, 12, 48, 2)):
        assert L.bk_grad_set_cnn2(FAKE, None, 0, 0, None, shape(*ok)) == _lib.BK_EINVAL and "nn >= 1" in _lib.last_error()


def test_set_refusals_in_order():
    L = _lib.lib()
    X, y = np.zeros((3, DIN), np.float32), np.array([0, 2, 1], np.int32)
    xp, yp, sh, E = X.ctypes.data, y.ctypes.data, shape(*LFW), _lib.BK_EINVAL
    assert L.bk_grad_set_cnn2(None, xp, 3, DIN, yp, sh) == E
    assert L.bk_grad_set_cnn2(FAKE, xp, 3, DIN, yp, None) == E
    for nn, ldx, x_, y_, word in ((0, DIN, xp, yp, "nn >= 1"), (3, DIN - 1, xp, yp, "ldx=%d" % (DIN - 1)),
                                  (3, DIN, None, yp, "null X"), (3, DIN, xp, None, "null X"),
                                  (3, DIN, xp, yp, "y[1]=2")):
        assert L.bk_grad_set_cnn2(FAKE, x_, nn, ldx, y_, sh) == E and word in _lib.last_error()
    # the size before the pointers
    assert L.bk_grad_set_cnn2(FAKE, None, (1 << 31) + 1, DIN, None, sh) == _lib.BK_ENOTSUP


def test_call_refusals_in_order():
    L = _lib.lib()
    w, out, q = np.zeros(8), np.zeros(8), np.zeros(8, np.int64)
    wp, op, qp, H = w.ctypes.data, out.ctypes.data, q.ctypes.data, _lib.BK_HOST

    def call(ctx=FAKE, ww=wp, where=H, max_norm=100.0, prec=4, o=op, qq=qp):
        return L.bk_grad_cnn2(ctx, ww, where, None, 0, max_norm, None, prec, o, qq, None, None)

    for kw, word in ((dict(ctx=None), "null context"), (dict(ww=None), "null ww"),
                     (dict(o=None), "null delta_out"), (dict(where=7), "bad where"),
                     (dict(prec=19), "exceeds 18"), (dict(prec=-1), "without a precision"),
                     (dict(max_norm=0.0), "max_norm"), (dict(max_norm=float("nan")), "max_norm"),
                     (dict(max_norm=float("inf")), "max_norm")):
        assert call(**kw) == _lib.BK_EINVAL and word in _lib.last_error(), kw
    assert call(ww=None, max_norm=0.0) == _lib.BK_EINVAL and "null ww" in _lib.last_error()
