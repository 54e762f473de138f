"""The bk_commit_* family without a GPU: the prototypes in include/bk.h, the
bindings in the built library, the unchanged ABI version and kernel count, the
new sources in the build, every argument check that needs no state (nor a
context's GPU), the Python wrappers' validation and the Go shim's functions."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_commit_set_key": "bk_ctx *ctx, const uint8_t *pk, int64_t count",
    "bk_commit_key_count": "bk_ctx *ctx, int64_t *count",
    "bk_commit_msm": "bk_ctx *ctx, const int64_t *scalars, int where, int64_t n, int64_t key_first, "
                     "uint8_t *out64",
    "bk_commit_verify": "bk_ctx *ctx, const int64_t *scalars, int where, int64_t n, "
                        "int64_t key_first, const uint8_t *committed64, int *ok",
    "bk_commit_generate": "bk_ctx *ctx, const double *delta, const int64_t *q, int where, int64_t d, "
                          "int precision, int poly_size, int total_shares, uint8_t *commit_out, "
                          "uint8_t *chunk_out, uint8_t *witness_out",
    "bk_commit_stats": "bk_ctx *ctx, int64_t out[4]",
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


def test_sources_are_built():
    for s in ("bk_commit.hip", "bk_commit_api.hip"):
        assert s in build.SOURCES
        assert os.path.exists(os.path.join(build.CSRC, s))
    assert os.path.exists(os.path.join(build.CSRC, "bk_bn256.h"))
    assert "-ffp-contract=off" in build.FLAGS


def _fresh_message(call, word, status=_lib.BK_EINVAL):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == status
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, (word, msg)


class _Args:
    """Valid arguments for every entry, kept alive."""

    def __init__(self):
        self.pk = np.zeros((25, 64), dtype=np.uint8)
        self.q = np.zeros(25, dtype=np.int64)
        self.v = np.zeros(25)
        self.o = np.full(64, 7, dtype=np.uint8)
        self.ch = np.full((3, 64), 7, dtype=np.uint8)
        self.wi = np.full((3, 20, 64), 7, dtype=np.uint8)
        self.n = ctypes.c_int64(-5)
        self.ok = ctypes.c_int(-5)
        self.st = (ctypes.c_int64 * 4)(9, 9, 9, 9)


def test_null_context_is_einval():
    L = _lib.lib()
    a = _Args()
    H = _lib.BK_HOST
    qp, vp, op = a.q.ctypes.data, a.v.ctypes.data, a.o.ctypes.data
    for call in (lambda: L.bk_commit_set_key(None, a.pk.ctypes.data, 25),
                 lambda: L.bk_commit_key_count(None, ctypes.byref(a.n)),
                 lambda: L.bk_commit_msm(None, qp, H, 25, 0, op),
                 lambda: L.bk_commit_verify(None, qp, H, 25, 0, op, ctypes.byref(a.ok)),
                 lambda: L.bk_commit_generate(None, vp, None, H, 25, 4, 10, 20, op,
                                              a.ch.ctypes.data, a.wi.ctypes.data),
                 lambda: L.bk_commit_stats(None, a.st),
                 # whatever else is wrong with the call, the context is checked first
                 lambda: L.bk_commit_set_key(None, None, 0),
                 lambda: L.bk_commit_msm(None, None, 9, 0, -1, None),
                 lambda: L.bk_commit_verify(None, None, 9, 0, -1, None, None),
                 lambda: L.bk_commit_generate(None, None, None, 9, 0, 99, 0, 0, None, None, None),
                 lambda: L.bk_commit_stats(None, None)):
        _fresh_message(call, "null context")
    assert a.n.value == -5 and a.ok.value == -5 and list(a.st) == [9, 9, 9, 9]
    assert (a.o == 7).all()


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
    qp, vp, op = a.q.ctypes.data, a.v.ctypes.data, a.o.ctypes.data
    cp, wp = a.ch.ctypes.data, a.wi.ctypes.data
    okp = ctypes.byref(a.ok)

    def msm(s=qp, where=H, n=25, first=0, out=op):
        return lambda: L.bk_commit_msm(fake, s, where, n, first, out)

    def ver(s=qp, where=H, n=25, first=0, com=op, ok=okp):
        return lambda: L.bk_commit_verify(fake, s, where, n, first, com, ok)

    def gen(delta=vp, q=None, where=H, d=25, prec=4, poly=10, T=20, c=op, k=cp, w=wp):
        return lambda: L.bk_commit_generate(fake, delta, q, where, d, prec, poly, T, c, k, w)

    E, U = _lib.BK_EINVAL, _lib.BK_ENOTSUP
    cases = [
        (lambda: L.bk_commit_set_key(fake, None, 25), "null pk", E),
        (lambda: L.bk_commit_set_key(fake, a.pk.ctypes.data, 0), "count=0", E),
        (lambda: L.bk_commit_set_key(fake, a.pk.ctypes.data, -3), "count=-3", E),
        (lambda: L.bk_commit_set_key(fake, a.pk.ctypes.data, (1 << 22) + 1), "count=4194305", E),
        (lambda: L.bk_commit_key_count(fake, None), "null count", E),
        (msm(s=None), "null scalars", E),
        (msm(where=3), "where=3", E),
        (msm(where=-1), "where=-1", E),
        (msm(n=0), "n=0", E),
        (msm(n=-2), "n=-2", E),
        (msm(first=-1), "key_first=-1", E),
        (msm(out=None), "null out64", E),
        (ver(s=None), "null scalars", E),
        (ver(where=5), "where=5", E),
        (ver(n=0), "n=0", E),
        (ver(first=-4), "key_first=-4", E),
        (ver(com=None), "null committed64", E),
        (ver(ok=None), "null ok", E),
        (gen(delta=None), "neither delta nor q", E),
        (gen(q=qp), "both delta and q", E),
        (gen(where=3), "where=3", E),
        (gen(d=0), "d=0", E),
        (gen(d=-4), "d=-4", E),
        (gen(prec=19), "precision=19", U),
        (gen(prec=-1), "precision=-1", U),
        (gen(poly=0), "poly_size=0", U),
        (gen(poly=11), "poly_size=11", U),
        (gen(T=9), "total_shares=9", U),
        (gen(T=65), "total_shares=65", U),
        (gen(c=None, k=None, w=None), "no output", E),
        (lambda: L.bk_commit_stats(fake, None), "null out", E),
    ]
    for call, word, status in cases:
        _fresh_message(call, word, status)
    assert a.ok.value == -5 and a.n.value == -5 and (a.o == 7).all()


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
    q = np.zeros(25, dtype=np.int64)
    v = np.zeros(25)
    calls = [
        lambda: e.commit_set_key(b"\0" * 63),
        lambda: e.commit_set_key(b""),
        lambda: e.commit_set_key(np.zeros((3, 32), dtype=np.uint8)),
        lambda: e.commit_set_key(np.zeros(64, dtype=np.int8)),
        # no key yet
        lambda: e.commit_msm(q),
        lambda: e.commit_verify(q, bytes(64)),
        lambda: e.commit_generate(v),
    ]
    for bad_call in calls:
        with pytest.raises(ValueError) as ei:
            bad_call()
        assert "null context" not in str(ei.value)
    e._commit_key = 30
    for bad_call in (
            lambda: e.commit_msm(q.astype(np.int32)),
            lambda: e.commit_msm(np.zeros((5, 5), dtype=np.int64)),
            lambda: e.commit_msm(np.zeros(0, dtype=np.int64)),
            lambda: e.commit_msm(q, first=6),
            lambda: e.commit_msm(q, first=-1),
            lambda: e.commit_verify(q, bytes(63)),
            lambda: e.commit_verify(q, bytes(64), first=7),
            lambda: e.commit_generate(v.astype(np.float32)),
            lambda: e.commit_generate(np.zeros((5, 5))),
            lambda: e.commit_generate(np.zeros(0)),
            lambda: e.commit_generate(np.zeros(31)),
            lambda: e.commit_generate(v, precision=19),
            lambda: e.commit_generate(v, poly_size=11),
            lambda: e.commit_generate(v, total_shares=9),
            lambda: e.commit_generate(v, total_shares=65),
            lambda: e.commit_generate(v, want_commit=False, want_chunks=False,
                                      want_witnesses=False)):
        with pytest.raises(ValueError) as ei:
            bad_call()
        assert "null context" not in str(ei.value)


def test_commit_module_surface():
    from biscotti_amd import commit
    for name in ("CommitKey", "create_commitment", "verify_commitment",
                 "generate_miner_commitments"):
        assert name in commit.__all__ and callable(getattr(commit, name)), name
    for name in ("from_points", "create_commitment", "verify_commitment",
                 "generate_miner_commitments"):
        assert callable(getattr(commit.CommitKey, name)), name
    with pytest.raises(ValueError):
        commit.create_commitment(object(), np.zeros(3, dtype=np.int64))


def test_go_shim_has_the_commitments():
    import go_shim_check as G
    go = open(G.SHIM).read()
    funcs = {name for name, _, _ in G._functions(go)}
    assert {"setCommitKeyGPU", "createCommitmentGPU", "verifyCommitmentGPU",
            "fillPolynomialMapGPU"} <= funcs
    used = {name for name, _, _ in G.shim_calls(go)}
    assert {"bk_commit_set_key", "bk_commit_msm", "bk_commit_verify", "bk_commit_generate"} <= used
    # names and arity, then the calls' types compiled against bk.h as it stands
    header = open(G.HEADER).read()
    assert G.check_names(go, header) == []
    ok, diag, _ = G.compile_check(go, os.path.dirname(G.HEADER))
    assert ok, diag
