"""The one-layer cifar CNN's entries without a GPU: the prototypes in
include/bk.h against the bindings, the unchanged ABI version and kernel-id
count, and every refusal that needs no GPU state (they all return before the
context is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "bk_eval_set_cnnc": "bk_ctx *ctx, int set, const float *X, int64_t nv, int64_t ldv, "
                        "const int32_t *y, const bk_cnnc_shape *shape",
    "bk_roni_cnnc_set_validation": "bk_ctx *ctx, const float *Xv, int64_t nv, int64_t ldv, "
                                   "const int32_t *yv, const bk_cnnc_shape *shape",
    "bk_roni_cnnc_batches": "bk_ctx *ctx, const double *ww, const double *deltas, int64_t n, "
                            "int64_t ld, const int64_t *idx, int64_t nb, double *scores, "
                            "int32_t *near_ties",
}
CIFAR = (3, 32, 32, 3, 3, 20, 10)
FAKE = ctypes.c_void_p(64)  # a context no refused call may touch


def shape(*v):
    return (ctypes.c_int32 * 7)(*v)


def set_calls(sh, nv=1):
    """Both set entries on a zero image; an accepted shape is refused for its nv = 0."""
    L = _lib.lib()
    X, y = np.zeros((1, 4 * 64 * 64), np.float32), np.zeros(1, np.int32)
    return {L.bk_eval_set_cnnc(FAKE, 0, X.ctypes.data, nv, X.shape[1], y.ctypes.data, shape(*sh)),
            L.bk_roni_cnnc_set_validation(FAKE, X.ctypes.data, nv, X.shape[1], y.ctypes.data, shape(*sh))}


def test_prototypes_and_bindings():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION and len(_lib.ALL_KERNELS) == 21
    assert re.search(r"typedef struct bk_cnnc_shape \{\s*int32_t c_in, h, w, k, pad, c_out, n_classes;", text)
    for name, want in PROTOS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m and re.sub(r"\s+", " ", m.group(1)).strip() == want
        res, args = _lib.SIGNATURES[name]
        assert hasattr(L, name) and res is ctypes.c_int and len(args) == want.count(",") + 1
    assert {"bk_cnnc.hip", "bk_cnnc_api.hip"} <= set(build.SOURCES)


# each bound of bk.h on both sides: (field, the last value inside, the first outside)
@pytest.mark.parametrize("field,inside,outside", [
    (0, 1, 0), (0, 4, 5), (1, 1, 0), (1, 64, 65), (2, 1, 0), (2, 64, 65), (3, 1, 0), (3, 5, 6),
    (4, 0, -1), (4, 3, 4),  # pad = k is accepted, pad = k + 1 refused
    (5, 1, 0), (5, 32, 33), (6, 2, 1), (6, 16, 17)])
def test_shape_limits(field, inside, outside):
    base = [1, 8, 8, 3, 1, 4, 10]
    ok, bad = list(base), list(base)
    ok[field], bad[field] = inside, outside
    if field == 3:  # pad <= k is a bound of its own
        ok[4] = bad[4] = 0
    assert set_calls(bad) == {_lib.BK_ENOTSUP} and "outside" in _lib.last_error()
    assert set_calls(ok, nv=0) == {_lib.BK_EINVAL} and "nv" in _lib.last_error()


def test_kernel_larger_than_padded_image_and_lds():
    assert set_calls((1, 1, 4, 5, 1, 4, 2)) == {_lib.BK_ENOTSUP}  # k = 5 > h + 2 pad = 3
    assert set_calls((1, 4, 1, 5, 1, 4, 2)) == {_lib.BK_ENOTSUP}
    assert set_calls(CIFAR, nv=0) == {_lib.BK_EINVAL}
    assert set_calls((4, 64, 64, 5, 5, 32, 10)) == {_lib.BK_ENOTSUP}  # the band ring exceeds the LDS
    assert "LDS" in _lib.last_error()


def test_refusals():
    L = _lib.lib()
    din = 3 * 32 * 32
    X, y = np.zeros((3, din), np.float32), np.array([0, 10, 1], np.int32)
    xp, yp, sh, E = X.ctypes.data, y.ctypes.data, shape(*CIFAR), _lib.BK_EINVAL
    assert L.bk_eval_set_cnnc(None, 0, xp, 3, din, yp, sh) == E
    assert L.bk_roni_cnnc_set_validation(None, xp, 3, din, yp, sh) == E
    assert L.bk_roni_cnnc_batches(None, xp, xp, 1, 1, xp, 1, xp, None) == E
    assert L.bk_roni_cnnc_batches(FAKE, xp, xp, 1, 1, None, 1, xp, None) == E
    for st in (4, -1):
        assert L.bk_eval_set_cnnc(FAKE, st, xp, 3, din, yp, sh) == E
    assert L.bk_eval_set_cnnc(FAKE, 0, xp, 3, din, yp, None) == E
    for nv, ldv, x_, y_ in ((0, din, xp, yp), (3, din - 1, xp, yp), (3, din, None, yp), (3, din, xp, None)):
        assert L.bk_eval_set_cnnc(FAKE, 0, x_, nv, ldv, y_, sh) == E
        assert L.bk_roni_cnnc_set_validation(FAKE, x_, nv, ldv, y_, sh) == E
    assert L.bk_eval_set_cnnc(FAKE, 0, xp, 3, din, yp, sh) == E  # the label names its sample
    assert "y[1]=10" in _lib.last_error()
