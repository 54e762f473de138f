"""The bk_shares_* family without a GPU: the prototypes in include/bk.h, the
bindings in the built library, the unchanged ABI version and kernel count, both
new sources in the build, every argument check that needs no state (nor a
context's GPU), the Python wrappers' validation and the Go shim's functions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_shares_chunks": "int64_t d, int poly_size",
    "bk_shares_generate": "bk_ctx *ctx, const double *delta, int where, int64_t d, int precision, "
                          "int poly_size, int total_shares, int64_t *y_out",
    "bk_shares_begin": "bk_ctx *ctx, int64_t d, int poly_size, int held, int64_t n_cap",
    "bk_shares_add": "bk_ctx *ctx, const int64_t *part, int where, int64_t *slot",
    "bk_shares_count": "bk_ctx *ctx, int64_t *count",
    "bk_shares_sum": "bk_ctx *ctx, const int64_t *slots, int64_t count, int64_t *sum_out",
    "bk_shares_recover": "bk_ctx *ctx, const int64_t *const *parts, const int *held, "
                         "const int64_t *xs, int nparts, int where, int64_t d, int poly_size, "
                         "int precision, const double *global_w, int64_t *coef_out, "
                         "double *delta_out, double *global_out, int64_t *bad_chunks",
    "bk_shares_stats": "bk_ctx *ctx, int64_t out[4]",
}


def _header():
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def _proto(name):
    m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
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
        assert res is (ctypes.c_int64 if name == "bk_shares_chunks" else ctypes.c_int)
        assert len(args) == want.count(",") + 1
        if name != "bk_shares_chunks":
            assert args[0] is ctypes.c_void_p
    text = _header()
    assert re.search(r"#define\s+BK_SHARES_MAX_POLY\s+10\b", text)
    assert re.search(r"#define\s+BK_SHARES_MAX_POINTS\s+64\b", text)
    assert (_lib.BK_SHARES_MAX_POLY, _lib.BK_SHARES_MAX_POINTS) == (10, 64)


def test_sources_are_built():
    assert "bk_shares.hip" in build.SOURCES and "bk_shares_api.hip" in build.SOURCES
    for s in ("bk_shares.hip", "bk_shares_api.hip"):
        assert os.path.exists(os.path.join(build.CSRC, s))
    assert "-ffp-contract=off" in build.FLAGS


def test_chunks():
    L = _lib.lib()
    assert L.bk_shares_chunks(1, 10) == 1
    assert L.bk_shares_chunks(25, 10) == 3
    assert L.bk_shares_chunks(2561, 10) == 257
    assert L.bk_shares_chunks(7850, 10) == 785
    assert L.bk_shares_chunks(7, 3) == 3
    assert L.bk_shares_chunks(0, 10) == -1 and "d=0" in _lib.last_error()
    assert L.bk_shares_chunks(5, 11) == -1 and "poly_size=11" in _lib.last_error()
    assert L.bk_shares_chunks(5, 0) == -1 and "poly_size=0" in _lib.last_error()


def _fresh_message(call, word):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == _lib.BK_EINVAL
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, (word, msg)


class _Args:
    """Valid arguments for every entry, kept alive."""

    def __init__(self):
        self.v = np.zeros(25)
        self.y = np.zeros((3, 20), dtype=np.int64)
        self.part = np.zeros((3, 20), dtype=np.int64)
        self.parts = (ctypes.c_void_p * 2)(self.part.ctypes.data, self.part.ctypes.data)
        self.held1 = np.array([20], dtype=np.intc)
        self.held2 = np.array([10, 10], dtype=np.intc)
        self.xs = np.arange(20, dtype=np.int64) - 10
        self.out = np.zeros(25)
        self.coef = np.zeros(25, dtype=np.int64)
        self.bad = ctypes.c_int64(-5)
        self.n = ctypes.c_int64(-5)
        self.slots = np.zeros(1, dtype=np.int64)
        self.st = (ctypes.c_int64 * 4)(9, 9, 9, 9)


def test_null_context_is_einval():
    L = _lib.lib()
    a = _Args()
    H = _lib.BK_HOST
    vp, yp, pp = a.v.ctypes.data, a.y.ctypes.data, a.part.ctypes.data
    for call in (lambda: L.bk_shares_generate(None, vp, H, 25, 4, 10, 20, yp),
                 lambda: L.bk_shares_begin(None, 25, 10, 5, 35),
                 lambda: L.bk_shares_add(None, pp, H, None),
                 lambda: L.bk_shares_count(None, ctypes.byref(a.n)),
                 lambda: L.bk_shares_sum(None, a.slots.ctypes.data, 1, None),
                 lambda: L.bk_shares_recover(None, a.parts, a.held2.ctypes.data, a.xs.ctypes.data, 2,
                                             H, 25, 10, 4, vp, None, None, a.out.ctypes.data,
                                             ctypes.byref(a.bad)),
                 lambda: L.bk_shares_stats(None, a.st),
                 # whatever else is wrong with the call, the context is checked first
                 lambda: L.bk_shares_generate(None, None, 9, 0, 99, 0, 0, None),
                 lambda: L.bk_shares_begin(None, 0, 0, 0, 0),
                 lambda: L.bk_shares_recover(None, None, None, None, 0, 9, 0, 0, 99, None, None,
                                             None, None, None),
                 lambda: L.bk_shares_stats(None, None)):
        _fresh_message(call, "null context")
    assert a.n.value == -5 and a.bad.value == -5 and list(a.st) == [9, 9, 9, 9]


# The checks behind the context: the entries never dereference the handle before
# they have passed, so a context that was never created stands in for one.  It
# is only ever refused.
class _Ctx(ctypes.Structure):
    _fields_ = [("pad", ctypes.c_char * 1)]


def test_bad_arguments_need_no_state():
    L = _lib.lib()
    a = _Args()
    keep = _Ctx()
    fake = ctypes.addressof(keep)
    H = _lib.BK_HOST
    vp, yp, pp, op = a.v.ctypes.data, a.y.ctypes.data, a.part.ctypes.data, a.out.ctypes.data
    h1, h2, xp = a.held1.ctypes.data, a.held2.ctypes.data, a.xs.ctypes.data
    bad = ctypes.byref(a.bad)

    def gen(delta=vp, where=H, d=25, prec=4, poly=10, T=20, y=yp):
        return lambda: L.bk_shares_generate(fake, delta, where, d, prec, poly, T, y)

    def rec(parts=a.parts, held=h2, xs=xp, nparts=2, where=H, d=25, poly=10, prec=4, w=vp,
            out=op, badp=bad):
        return lambda: L.bk_shares_recover(fake, parts, held, xs, nparts, where, d, poly, prec, w,
                                           None, None, out, badp)

    held_bad = np.array([10, 0], dtype=np.intc)
    held_few = np.array([4, 5], dtype=np.intc)
    held_many = np.array([40, 30], dtype=np.intc)
    xs_dup = a.xs.copy()
    xs_dup[7] = xs_dup[2]
    xs_far = a.xs.copy()
    xs_far[3] = 54
    xs_low = a.xs.copy()
    xs_low[0] = -11
    two_null = (ctypes.c_void_p * 2)(None, None)
    cases = [
        (gen(delta=None), "null delta"),
        (gen(where=3), "where=3"),
        (gen(where=-1), "where=-1"),
        (gen(d=0), "d=0"),
        (gen(d=-4), "d=-4"),
        (gen(d=(1 << 30) + 1), "d=1073741825"),
        (gen(prec=19), "precision=19"),
        (gen(prec=-1), "precision=-1"),
        (gen(poly=0), "poly_size=0"),
        (gen(poly=11), "poly_size=11"),
        (gen(T=9), "total_shares=9"),
        (gen(T=65), "total_shares=65"),
        (gen(y=None), "null y_out"),
        (lambda: L.bk_shares_begin(fake, 0, 10, 5, 35), "d=0"),
        (lambda: L.bk_shares_begin(fake, 25, 12, 5, 35), "poly_size=12"),
        (lambda: L.bk_shares_begin(fake, 25, 10, 0, 35), "held=0"),
        (lambda: L.bk_shares_begin(fake, 25, 10, 65, 35), "held=65"),
        (lambda: L.bk_shares_begin(fake, 25, 10, 5, 0), "n_cap=0"),
        (lambda: L.bk_shares_begin(fake, 25, 10, 5, _lib.BK_MAX_N + 1), "n_cap=16385"),
        (lambda: L.bk_shares_add(fake, None, H, None), "null part"),
        (lambda: L.bk_shares_add(fake, pp, 7, None), "where=7"),
        (lambda: L.bk_shares_count(fake, None), "null count"),
        (lambda: L.bk_shares_sum(fake, None, 1, None), "null slots"),
        (lambda: L.bk_shares_sum(fake, a.slots.ctypes.data, 0, None), "count=0"),
        (lambda: L.bk_shares_sum(fake, a.slots.ctypes.data, -2, None), "count=-2"),
        (rec(parts=None), "null parts"),
        (rec(held=None), "null held"),
        (rec(xs=None), "null xs"),
        (rec(nparts=0), "nparts=0"),
        (rec(nparts=65), "nparts=65"),
        (rec(where=4), "where=4"),
        (rec(d=0), "d=0"),
        (rec(poly=11), "poly_size=11"),
        (rec(prec=19), "precision=19"),
        (rec(w=None), "null global_w"),
        (rec(out=None), "null global_out"),
        (rec(badp=None), "null bad_chunks"),
        (rec(held=held_bad.ctypes.data), "held[1]=0"),
        (rec(held=held_few.ctypes.data), "9 points"),
        (rec(held=held_many.ctypes.data), "70 points"),
        (rec(xs=xs_dup.ctypes.data), "xs[2] == xs[7]"),
        (rec(xs=xs_far.ctypes.data), "xs[3]=54"),
        (rec(xs=xs_low.ctypes.data), "xs[0]=-11"),
        (rec(parts=two_null), "at most one"),
        (lambda: L.bk_shares_stats(fake, None), "null out"),
    ]
    for call, word in cases:
        _fresh_message(call, word)
    assert a.bad.value == -5 and a.n.value == -5


class _NoLibEngine:
    """An Engine whose context is never made: the wrappers must refuse before
    the library is reached."""

    def __new__(cls):
        from biscotti_amd.krum import Engine
        e = object.__new__(Engine)
        e._ctx = None
        return e


def test_wrappers_validate_before_the_library():
    e = _NoLibEngine()
    v = np.zeros(25)
    part = np.zeros((3, 5), dtype=np.int64)
    xs = np.arange(20) - 10
    for bad_call in (
            lambda: e.shares_generate(np.zeros(25, dtype=np.float32)),
            lambda: e.shares_generate(np.zeros((5, 5))),
            lambda: e.shares_generate(np.zeros(0)),
            lambda: e.shares_generate(v, precision=19),
            lambda: e.shares_generate(v, poly_size=11),
            lambda: e.shares_generate(v, poly_size=0),
            lambda: e.shares_generate(v, total_shares=9),
            lambda: e.shares_generate(v, total_shares=65),
            lambda: e.shares_begin(0, 10, 5, 35),
            lambda: e.shares_begin(25, 11, 5, 35),
            lambda: e.shares_begin(25, 10, 0, 35),
            lambda: e.shares_begin(25, 10, 5, 0),
            lambda: e.shares_add(part),
            lambda: e.shares_sum(np.arange(3)),
            lambda: e.shares_recover(v.astype(np.float32), [part] * 4, xs),
            lambda: e.shares_recover(v, [], xs),
            lambda: e.shares_recover(v, [None, None, part, part], xs),
            lambda: e.shares_recover(v, [part.astype(np.int32)] * 4, xs),
            lambda: e.shares_recover(v, [part[:2]] * 4, xs),
            lambda: e.shares_recover(v, [part] * 4, xs[:19]),
            lambda: e.shares_recover(v, [part] * 4, xs.astype(np.float64)),
            lambda: e.shares_recover(v, [part] * 4, np.where(xs == 3, 2, xs)),
            lambda: e.shares_recover(v, [part], xs[:5]),
            lambda: e.shares_recover(v, [part] * 4, xs, precision=-1)):
        with pytest.raises(ValueError) as ei:
            bad_call()
        assert "null context" not in str(ei.value)
    # with a store's shape known, the part's shape and dtype are checked
    e._shares = (25, 10, 5, 3)
    for bad_part in (np.zeros((3, 4), dtype=np.int64), np.zeros((3, 5)), np.zeros(15, dtype=np.int64)):
        with pytest.raises(ValueError) as ei:
            e.shares_add(bad_part)
        assert "null context" not in str(ei.value)
    for bad_slots in (np.zeros(0, dtype=np.int64), np.zeros((2, 2), dtype=np.int64), np.zeros(3)):
        with pytest.raises(ValueError) as ei:
            e.shares_sum(bad_slots)
        assert "null context" not in str(ei.value)


def test_shares_module_surface():
    from biscotti_amd import shares
    for name in ("generate_miner_shares", "ShareStore", "recover_block", "miner_nodes",
                 "shares_per_miner"):
        assert name in shares.__all__ and callable(getattr(shares, name)), name
    for name in ("add_part", "miner_part"):
        assert callable(getattr(shares.ShareStore, name)), name
    assert shares.shares_per_miner(20, 4) == 5 and shares.shares_per_miner(21, 3) == 7
    with pytest.raises(ValueError):
        shares.shares_per_miner(20, 3)
    assert shares.miner_nodes(2, 5).tolist() == [0, 1, 2, 3, 4]


def test_go_shim_has_the_secure_path():
    import go_shim_check as G
    go = open(G.SHIM).read()
    funcs = {name for name, _, _ in G._functions(go)}
    assert {"generateSharesGPU", "addSecretShareGPU", "getMinerPartGPU",
            "recoverAggregateGPU"} <= funcs
    used = {name for name, _, _ in G.shim_calls(go)}
    assert {"bk_shares_generate", "bk_shares_begin", "bk_shares_add", "bk_shares_sum"} <= used
    # bk_shares_recover's `const int64_t *const *` is reached through a C helper
    # in the cgo preamble (cgo has no conversion to that type from a C-allocated
    # pointer table that the call rewriting understands): the preamble is C, so
    # it is compiled against bk.h as it stands
    pre = re.search(r"/\*\n(#cgo.*?)\*/\nimport \"C\"", go, re.S).group(1)
    pre = re.sub(r"^#cgo.*$", "", pre, flags=re.M)
    assert "bk_shares_recover(" in pre
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function",
                        "-I" + os.path.dirname(G.HEADER), "-x", "c", "-"], input=pre,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
