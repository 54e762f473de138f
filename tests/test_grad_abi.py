"""The bk_grad_* family without a GPU: the prototypes in include/bk.h, the
bindings in the built library, the unchanged ABI version and kernel count, both
new sources in the build, every argument check that needs no resident set (nor
a context's GPU) in the documented order, the steppers' validation and the Go
shim's functions."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_grad_set_logistic": "bk_ctx *ctx, const double *X, int64_t nn, int64_t d, int64_t ldx, "
                            "const double *y",
    "bk_grad_set_softmax": "bk_ctx *ctx, const float *X, int64_t nn, int64_t d_in, int64_t ldx, "
                           "const int32_t *y, int64_t n_classes",
    "bk_grad_clear": "bk_ctx *ctx",
    "bk_grad_logistic": "bk_ctx *ctx, const double *ww, int where, const int64_t *idx, "
                        "int64_t count, int64_t batch_size, double alpha, double lammy, "
                        "const double *noise, int precision, double *delta_out, int64_t *q_out, "
                        "double *loss_out",
    "bk_grad_softmax": "bk_ctx *ctx, const double *ww, int where, const int64_t *idx, "
                       "int64_t count, double max_norm, const double *noise, int precision, "
                       "double *delta_out, int64_t *q_out, double *loss_out, double *norm_out",
    "bk_grad_stats": "bk_ctx *ctx, int64_t out[2]",
}


def _header():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def _proto(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototypes_and_bindings():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    assert len(_lib.ALL_KERNELS) == 21
    for name, want in PROTOS.items():
        assert _proto(name) == want
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == want.count(",") + 1
        assert args[0] is ctypes.c_void_p
    assert (_lib.BK_GRAD_MAX_BATCH, _lib.BK_GRAD_MAX_D) == (65536, 32768)


def test_sources_are_built():
    assert "bk_grad.hip" in build.SOURCES and "bk_grad_api.hip" in build.SOURCES
    for s in ("bk_grad.hip", "bk_grad_api.hip"):
        assert os.path.exists(os.path.join(build.CSRC, s))
    assert "-ffp-contract=off" in build.FLAGS
    ctx = open(os.path.join(build.CSRC, "bk_ctx.h")).read()
    assert re.search(r"\bstruct Grad\s*\{", ctx)


def _message(call, code, word):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == code
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, (word, msg)


# The checks behind the null context never dereference the handle before they
# have passed, so a context that was never created stands in for one.  It is
# only ever refused.
class _Ctx(ctypes.Structure):
    _fields_ = [("pad", ctypes.c_char * 1)]


class _Args:
    def __init__(self):
        self.w = np.zeros(25)
        self.out = np.zeros(25)
        self.q = np.zeros(25, dtype=np.int64)
        self.idx = np.arange(10, dtype=np.int64)
        self.X = np.zeros((4, 25))
        self.y = np.ones(4)
        self.Xf = np.zeros((4, 24), dtype=np.float32)
        self.yi = np.array([0, 1, 1, 0], dtype=np.int32)
        self.st = (ctypes.c_int64 * 2)(9, 9)


def _logistic(L, ctx, a, ww="w", where=_lib.BK_HOST, count=10, batch=10, prec=4, out="out", q="q"):
    g = lambda n: getattr(a, n).ctypes.data if n else None  # noqa: E731
    return lambda: L.bk_grad_logistic(ctx, g(ww), where, a.idx.ctypes.data, count, batch, 1e-2, 0.01,
                                      None, prec, g(out), g(q), None)


def _softmax(L, ctx, a, ww="w", where=_lib.BK_HOST, count=10, max_norm=100.0, prec=4, out="out",
             q="q"):
    g = lambda n: getattr(a, n).ctypes.data if n else None  # noqa: E731
    return lambda: L.bk_grad_softmax(ctx, g(ww), where, a.idx.ctypes.data, count, max_norm, None,
                                     prec, g(out), g(q), None, None)


def test_null_context_is_checked_first():
    L = _lib.lib()
    a = _Args()
    for call in (lambda: L.bk_grad_set_logistic(None, a.X.ctypes.data, 4, 25, 25, a.y.ctypes.data),
                 lambda: L.bk_grad_set_softmax(None, a.Xf.ctypes.data, 4, 24, 24, a.yi.ctypes.data, 2),
                 lambda: L.bk_grad_clear(None),
                 _logistic(L, None, a),
                 _softmax(L, None, a),
                 lambda: L.bk_grad_stats(None, a.st),
                 # whatever else is wrong with the call
                 lambda: L.bk_grad_set_softmax(None, None, 0, 0, 0, None, 99),
                 _logistic(L, None, a, ww=None, where=9, batch=0, prec=99, out=None),
                 _softmax(L, None, a, ww=None, where=9, max_norm=-1.0, prec=99, out=None),
                 lambda: L.bk_grad_stats(None, None)):
        _message(call, _lib.BK_EINVAL, "null context")
    assert list(a.st) == [9, 9]


def test_call_checks_in_order_need_no_state():
    L = _lib.lib()
    a = _Args()
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    E = _lib.BK_EINVAL
    for fam in (_logistic, _softmax):
        own = dict(batch=0) if fam is _logistic else dict(max_norm=0.0)
        cases = [
            # check 1 comes before 2 and 3
            (fam(L, fake, a, ww=None, prec=19, **own), "null ww"),
            (fam(L, fake, a, out=None, prec=19, **own), "null delta_out"),
            (fam(L, fake, a, where=3, prec=19, **own), "where=3"),
            (fam(L, fake, a, where=-1), "where=-1"),
            # check 2 comes before 3
            (fam(L, fake, a, prec=19, **own), "precision=19"),
            (fam(L, fake, a, prec=-1, **own), "q_out without a precision"),
        ]
        for call, word in cases:
            _message(call, E, word)
    # check 3
    _message(_logistic(L, fake, a, batch=0), E, "batch_size=0")
    _message(_logistic(L, fake, a, batch=-3, count=0), E, "batch_size=-3")
    for mn in (0.0, -1.0, float("inf"), float("nan")):
        _message(_softmax(L, fake, a, max_norm=mn, count=0), E, "max_norm=")
    _message(lambda: L.bk_grad_stats(fake, None), E, "null out")
    assert not a.out.any() and not a.q.any()


def test_set_checks_need_no_state():
    L = _lib.lib()
    a = _Args()
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    E, N = _lib.BK_EINVAL, _lib.BK_ENOTSUP
    Xp, yp, Xfp, yip = a.X.ctypes.data, a.y.ctypes.data, a.Xf.ctypes.data, a.yi.ctypes.data
    bad_label = np.array([0, 1, 2, 0], dtype=np.int32)

    def lg(X=Xp, nn=4, d=25, ldx=25, y=yp):
        return lambda: L.bk_grad_set_logistic(fake, X, nn, d, ldx, y)

    def sm(X=Xfp, nn=4, din=24, ldx=24, y=yip, C=2):
        return lambda: L.bk_grad_set_softmax(fake, X, nn, din, ldx, y, C)

    cases = [
        (lg(nn=0), E, "nn=0"), (lg(d=0), E, "d=0"), (lg(ldx=24), E, "ldx=24"),
        (lg(X=None), E, "null X"), (lg(y=None), E, "null X / y"),
        # BK_EINVAL before BK_ENOTSUP
        (lg(X=None, d=32769, ldx=32769), E, "null X"),
        (lg(d=32769, ldx=32769), N, "d=32769"),
        (lg(nn=(1 << 31) + 1), N, "too large"),
        (sm(nn=0), E, "nn=0"), (sm(din=0), E, "d=0"), (sm(ldx=23), E, "ldx=23"),
        (sm(C=1), E, "n_classes=1"), (sm(X=None), E, "null X"), (sm(y=None), E, "null X / y"),
        (sm(y=bad_label.ctypes.data), E, "y[2]=2"),
        (sm(X=None, C=17), E, "null X"),
        (sm(C=17), N, "n_classes=17"),
        (sm(din=32769, ldx=32769), N, "d_in=32769"),
    ]
    for call, code, word in cases:
        _message(call, code, word)


class _NoLibEngine:
    """An Engine whose context is never made: the wrappers must refuse before
    the library is reached."""

    def __new__(cls):
        from biscotti_amd.krum import Engine
        e = object.__new__(Engine)
        e._ctx = None
        return e


def test_steppers_validate_before_the_library():
    from biscotti_amd.train import LogisticStepper, SoftmaxStepper
    e = _NoLibEngine()
    X = np.zeros((6, 5))
    y = np.array([1, -1, 1, 1, -1, 1])
    Xf = np.zeros((6, 4), dtype=np.float32)
    yi = np.array([0, 1, 2, 1, 0, 2])
    for bad in (lambda: LogisticStepper(X.astype(np.float32), y, 3, engine=e),
                lambda: LogisticStepper(X[0], y, 3, engine=e),
                lambda: LogisticStepper(X, y[:5], 3, engine=e),
                lambda: LogisticStepper(X, np.array(["a"] * 6), 3, engine=e),
                lambda: LogisticStepper(X, np.where(y > 0, np.nan, 1.0), 3, engine=e),
                lambda: LogisticStepper(X, y, 0, engine=e),
                lambda: LogisticStepper(np.zeros((0, 5)), y[:0], 3, engine=e),
                lambda: SoftmaxStepper(Xf.astype(np.float64), yi, 3, engine=e),
                lambda: SoftmaxStepper(Xf, yi.astype(np.float64), 3, engine=e),
                lambda: SoftmaxStepper(Xf, yi, 2, engine=e),
                lambda: SoftmaxStepper(Xf, -yi, 3, engine=e),
                lambda: SoftmaxStepper(Xf, yi, 1, engine=e),
                lambda: SoftmaxStepper(Xf, yi, 17, engine=e),
                lambda: SoftmaxStepper(Xf, yi[:3], 3, engine=e),
                lambda: SoftmaxStepper(Xf, yi, 3, max_norm=0.0, engine=e),
                lambda: SoftmaxStepper(Xf, yi, 3, max_norm=float("nan"), engine=e)):
        with pytest.raises(ValueError) as ei:
            bad()
        assert "null context" not in str(ei.value)
    # a call's arguments, with a resident set's shape known
    e._grad = ("logistic", 6, 5)
    w = np.zeros(5)
    for bad in (lambda: e.grad_logistic(np.zeros(4)),
                lambda: e.grad_logistic(w, idx=np.zeros(0, dtype=np.int64)),
                lambda: e.grad_logistic(w, idx=np.array([0, 6])),
                lambda: e.grad_logistic(w, idx=np.array([-1])),
                lambda: e.grad_logistic(w, idx=np.array([0.0, 1.0])),
                lambda: e.grad_logistic(w, idx=np.zeros((2, 2), dtype=np.int64)),
                lambda: e.grad_logistic(w, batch_size=0),
                lambda: e.grad_logistic(w, noise=np.zeros(6)),
                lambda: e.grad_logistic(w, precision=19),
                lambda: e.grad_softmax(w),
                lambda: e.grad_logistic(w, idx=np.zeros(65537, dtype=np.int64))):
        with pytest.raises(ValueError) as ei:
            bad()
        assert "null context" not in str(ei.value)
    e._grad = ("softmax", 6, 15)
    for bad in (lambda: e.grad_softmax(np.zeros(15), max_norm=-1.0),
                lambda: e.grad_softmax(np.zeros(14)),
                lambda: e.grad_logistic(np.zeros(15))):
        with pytest.raises(ValueError):
            bad()


def test_train_module_surface():
    from biscotti_amd import train
    assert set(train.__all__) == {"LogisticStepper", "SoftmaxStepper"}
    for cls in (train.LogisticStepper, train.SoftmaxStepper):
        assert callable(cls.private_fun)
        assert cls.loss is None and cls.norm is None


def test_go_shim_has_the_gradient_step():
    import go_shim_check as G
    go = open(G.SHIM).read()
    funcs = {name for name, _, _ in G._functions(go)}
    assert {"initGradGPU", "oneGradientStepGPU"} <= funcs
    used = {name for name, _, _ in G.shim_calls(go)}
    assert {"bk_grad_set_logistic", "bk_grad_set_softmax", "bk_grad_logistic",
            "bk_grad_softmax"} <= used
    assert re.search(r"func oneGradientStepGPU\(globalW \[\]float64, idx \[\]int64\) "
                     r"\(\[\]float64, \[\]int64\)", go)
