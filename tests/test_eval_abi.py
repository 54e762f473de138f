"""The bk_eval* family and bk_block_finish_eval without a GPU: the prototypes in
include/bk.h, the bindings in the built library, the unchanged ABI version, every
argument check that needs no resident set, and the Python wrappers' shape and
dtype validation."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_eval_set_logistic": "bk_ctx *ctx, int set, const double *X, int64_t nv, int64_t d, "
                            "int64_t ldv, const double *y",
    "bk_eval_set_softmax": "bk_ctx *ctx, int set, const float *X, int64_t nv, int64_t d_in, "
                           "int64_t ldv, const int32_t *y, int64_t n_classes",
    "bk_eval_clear": "bk_ctx *ctx, int set",
    "bk_eval": "bk_ctx *ctx, const double *ww, int64_t d, int where, const int *sets, int nsets, "
               "double *err, int64_t *wrong, int32_t *near_ties",
    "bk_eval_stats": "bk_ctx *ctx, int64_t out[2]",
    "bk_block_finish_eval": "bk_ctx *ctx, double *global_out, int64_t *qsum_out, "
                            "double *qsum_float_out, const int *sets, int nsets, double *err, "
                            "int64_t *wrong, int32_t *near_ties",
}


def _proto(name):
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototypes_and_bindings():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    for name, want in PROTOS.items():
        assert _proto(name) == want
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == want.count(",") + 1 and args[0] is ctypes.c_void_p
    src = open(os.path.join(REPO, "include", "bk.h")).read()
    assert re.search(r"#define BK_EVAL_MAX_SETS 4\b", src) and _lib.BK_EVAL_MAX_SETS == 4


def test_source_list_and_shared_helpers():
    """bk_eval.hip is built, and the helpers it shares with bk_roni.hip live in
    one header that both include."""
    from biscotti_amd import build
    assert "bk_eval.hip" in build.SOURCES
    csrc = os.path.join(REPO, "biscotti_amd", "csrc")
    for f in ("bk_eval.hip", "bk_roni.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "bk_roni_dev.h"' in text
        assert "bool softmax_near_tie(" not in text and "bool round_exit(" not in text


def _fresh_message(call, word, code=_lib.BK_EINVAL):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == code
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, msg


class _Ctx(ctypes.Structure):
    _fields_ = [("pad", ctypes.c_char * 1)]


def _args():
    X = np.zeros((3, 4))
    Xf = np.zeros((3, 4), dtype=np.float32)
    y = np.zeros(3)
    yi = np.zeros(3, dtype=np.int32)
    w = np.zeros(4)
    sets = (ctypes.c_int * 4)(0, 1, 2, 3)
    err = np.zeros(4)
    wrong = np.zeros(4, dtype=np.int64)
    near = np.zeros(4, dtype=np.int32)
    return X, Xf, y, yi, w, sets, err, wrong, near


def test_null_context_is_einval():
    L = _lib.lib()
    X, Xf, y, yi, w, sets, err, wrong, near = _args()
    out = (ctypes.c_int64 * 2)(9, 9)
    H = _lib.BK_HOST
    for call in (
            lambda: L.bk_eval_set_logistic(None, 0, X.ctypes.data, 3, 4, 4, y.ctypes.data),
            lambda: L.bk_eval_set_softmax(None, 0, Xf.ctypes.data, 3, 4, 4, yi.ctypes.data, 2),
            lambda: L.bk_eval_clear(None, 0),
            lambda: L.bk_eval(None, w.ctypes.data, 4, H, sets, 1, err.ctypes.data,
                              wrong.ctypes.data, near.ctypes.data),
            lambda: L.bk_eval_stats(None, out),
            lambda: L.bk_block_finish_eval(None, w.ctypes.data, None, None, sets, 1,
                                           err.ctypes.data, wrong.ctypes.data, None),
            # whatever else is wrong with the call, the context is checked first
            lambda: L.bk_eval(None, None, 0, 9, None, 0, None, None, None),
            lambda: L.bk_eval_set_softmax(None, 7, None, 0, 0, 0, None, 99)):
        _fresh_message(call, "null context")
    assert list(out) == [9, 9]


def test_bad_arguments_need_no_set():
    """The checks behind the context never dereference the handle before they
    have passed: a context that was never created stands in for one."""
    L = _lib.lib()
    X, Xf, y, yi, w, sets, err, wrong, near = _args()
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    H = _lib.BK_HOST
    Xp, Xfp, yp, yip, wp = (a.ctypes.data for a in (X, Xf, y, yi, w))
    ep, rp, np_ = err.ctypes.data, wrong.ctypes.data, near.ctypes.data
    five = (ctypes.c_int * 5)(0, 1, 2, 3, 0)
    bad_hi = (ctypes.c_int * 2)(0, 4)
    bad_lo = (ctypes.c_int * 1)(-1)
    cases = [
        (lambda: L.bk_eval_set_logistic(fake, 4, Xp, 3, 4, 4, yp), "set=4"),
        (lambda: L.bk_eval_set_logistic(fake, -1, Xp, 3, 4, 4, yp), "set=-1"),
        (lambda: L.bk_eval_set_logistic(fake, 0, Xp, 0, 4, 4, yp), "nv=0"),
        (lambda: L.bk_eval_set_logistic(fake, 0, Xp, 3, 0, 4, yp), "d=0"),
        (lambda: L.bk_eval_set_logistic(fake, 0, Xp, 3, 4, 3, yp), "ldv=3"),
        (lambda: L.bk_eval_set_logistic(fake, 0, None, 3, 4, 4, yp), "null"),
        (lambda: L.bk_eval_set_logistic(fake, 0, Xp, 3, 4, 4, None), "null"),
        (lambda: L.bk_eval_set_softmax(fake, 5, Xfp, 3, 4, 4, yip, 2), "set=5"),
        (lambda: L.bk_eval_set_softmax(fake, 0, Xfp, -2, 4, 4, yip, 2), "nv=-2"),
        (lambda: L.bk_eval_set_softmax(fake, 0, Xfp, 3, 4, 2, yip, 2), "ldv=2"),
        (lambda: L.bk_eval_set_softmax(fake, 0, Xfp, 3, 4, 4, yip, 1), "n_classes=1"),
        (lambda: L.bk_eval_set_softmax(fake, 0, None, 3, 4, 4, yip, 2), "null"),
        (lambda: L.bk_eval_set_softmax(fake, 0, Xfp, 3, 4, 4, None, 2), "null"),
        (lambda: L.bk_eval_clear(fake, 4), "set=4"),
        (lambda: L.bk_eval(fake, None, 4, H, sets, 1, ep, rp, np_), "null ww"),
        (lambda: L.bk_eval(fake, wp, 4, H, None, 1, ep, rp, np_), "null"),
        (lambda: L.bk_eval(fake, wp, 4, H, sets, 1, None, rp, np_), "null"),
        (lambda: L.bk_eval(fake, wp, 4, H, sets, 1, ep, None, np_), "null"),
        (lambda: L.bk_eval(fake, wp, 4, H, sets, 0, ep, rp, np_), "nsets=0"),
        (lambda: L.bk_eval(fake, wp, 4, H, five, 5, ep, rp, np_), "nsets=5"),
        (lambda: L.bk_eval(fake, wp, 4, 3, sets, 1, ep, rp, np_), "where=3"),
        (lambda: L.bk_eval(fake, wp, 4, -1, sets, 1, ep, rp, None), "where=-1"),
        (lambda: L.bk_eval(fake, wp, 4, H, bad_hi, 2, ep, rp, np_), "set=4"),
        (lambda: L.bk_eval(fake, wp, 4, H, bad_lo, 1, ep, rp, np_), "set=-1"),
        (lambda: L.bk_eval_stats(fake, None), "null out"),
        (lambda: L.bk_block_finish_eval(fake, None, None, None, sets, 1, ep, rp, np_),
         "null global_out"),
    ]
    for call, word in cases:
        _fresh_message(call, word)
    _fresh_message(lambda: L.bk_eval_set_softmax(fake, 0, Xfp, 3, 4, 4, yip, 17), "n_classes=17",
                   _lib.BK_ENOTSUP)
    assert not err.any() and not wrong.any() and not near.any()


@pytest.mark.parametrize("pos,label", [(0, -1), (2, 3), (1, 1 << 20)])
def test_softmax_labels_are_range_checked(pos, label):
    L = _lib.lib()
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    Xf = np.zeros((3, 4), dtype=np.float32)
    yi = np.array([0, 2, 1], dtype=np.int32)
    yi[pos] = label
    _fresh_message(lambda: L.bk_eval_set_softmax(fake, 1, Xf.ctypes.data, 3, 4, 4, yi.ctypes.data, 3),
                   "y[%d]=%d" % (pos, label))


def _no_engine():
    """An Engine that was never created: the wrappers validate before they
    reach the library, which then refuses the null context."""
    from biscotti_amd.krum import Engine
    e = Engine.__new__(Engine)
    e._ctx = None
    return e


def test_engine_wrappers_validate_shapes_and_dtypes():
    e = _no_engine()
    X = np.zeros((5, 3))
    Xf = np.zeros((5, 3), dtype=np.float32)
    y = np.zeros(5)
    yi = np.zeros(5, dtype=np.int64)
    for bad in (lambda: e.eval_set_logistic(0, Xf, y),             # float32 samples
                lambda: e.eval_set_logistic(0, X[0], y),           # a vector
                lambda: e.eval_set_logistic(0, X, y[:4]),          # a label short
                lambda: e.eval_set_logistic(0, np.zeros((0, 3)), np.zeros(0)),
                lambda: e.eval_set_softmax(0, X, yi, 3),           # float64 samples
                lambda: e.eval_set_softmax(0, Xf, y, 3),           # float labels
                lambda: e.eval_set_softmax(0, Xf, yi[:3], 3),
                lambda: e.eval_set_softmax(0, Xf, yi + (1 << 40), 3),
                lambda: e.eval(np.zeros((2, 2)), [0]),
                lambda: e.eval(np.zeros(0), [0]),
                lambda: e.eval(np.zeros(3), []),
                lambda: e.eval(np.zeros(3), [0, 1, 2, 3, 0]),
                lambda: e.block_finish_eval([0])):                 # no block_begin
        with pytest.raises(ValueError) as ei:
            bad()
        assert "null context" not in str(ei.value)
    # valid arguments reach the library, which refuses the missing context
    for ok in (lambda: e.eval_set_logistic(0, X, y),
               lambda: e.eval_set_logistic(0, X[:, :2], y),        # a row stride is kept
               lambda: e.eval_set_softmax(1, Xf, yi, 3),
               lambda: e.eval(np.zeros(3), [0, 2]),
               lambda: e.eval_clear(0),
               lambda: e.eval_stats()):
        with pytest.raises(ValueError, match="null context"):
            ok()


def test_model_evaluator_validates_before_any_upload():
    from biscotti_amd import aggregate, evaluate
    import inspect
    e = _no_engine()
    X = np.zeros((5, 3))
    y = np.ones(5)
    M = evaluate.ModelEvaluator
    for bad in (lambda: M(engine=e),
                lambda: M(train=(X, y[:4]), engine=e),
                lambda: M(train=(X, y), test=(np.zeros((4, 2)), np.ones(4)), engine=e),
                lambda: M(train=(X[0], y), engine=e),
                lambda: M(train=(X, y), n_classes=1, engine=e),
                lambda: M(train=(X, y), n_classes=17, engine=e),
                lambda: M(train=(X,), engine=e)):
        with pytest.raises(ValueError) as ei:
            bad()
        assert "null context" not in str(ei.value)
    with pytest.raises(ValueError, match="null context"):
        M(train=(X, y), engine=e)
    for name in ("train_error", "test_error", "attack_rate", "check_convergence"):
        assert callable(getattr(M, name)), name
    assert (evaluate.TRAIN, evaluate.TEST, evaluate.ATTACK) == (0, 1, 2)
    sig = inspect.signature(aggregate.BlockCollector.create_block)
    assert sig.parameters["evaluator"].default is None


def test_goldens_are_small_and_hold_no_near_tie_seed_drift():
    """The committed fixtures: sizes, and the manifest agrees with the arrays."""
    import json
    gold = os.path.join(REPO, "tests", "golden")
    cases = json.load(open(os.path.join(gold, "eval_cases.json")))
    assert {"eval_credit_like", "eval_labels01", "eval_mnist", "eval_lfw", "eval_2class"} <= set(cases)
    for name, p in cases.items():
        path = os.path.join(gold, name + ".npz")
        assert os.path.getsize(path) < 512 * 1024
        with np.load(path, allow_pickle=False) as z:
            assert z["err"].tolist() == p["err"] and z["wrong"].tolist() == p["wrong"]
            if p["kind"] == "softmax":
                assert set(z["y_attack"].tolist()) == {1}  # the attack set: class 1 only
