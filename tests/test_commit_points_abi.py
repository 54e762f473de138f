"""The bk_commit_points_* family without a GPU: the prototypes in include/bk.h,
the bindings, the unchanged ABI version and kernel count, the new sources in the
build, every argument check that needs no state, the Python wrappers' validation
and the Go shim's functions."""
import ctypes
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = {
    "bk_commit_points_begin": "bk_ctx *ctx, int64_t chunks, int held, int64_t n_cap",
    "bk_commit_points_add": "bk_ctx *ctx, const uint8_t *commit64, const uint8_t *chunk_pts, "
                            "const uint8_t *witness_pts, int where, int64_t *slot",
    "bk_commit_points_count": "bk_ctx *ctx, int64_t *count",
    "bk_commit_points_set_lanes": "bk_ctx *ctx, int lanes",
    "bk_commit_points_sum": "bk_ctx *ctx, const int64_t *slots, int64_t count, int where, "
                            "uint8_t *commit_out, uint8_t *chunk_out, uint8_t *witness_out",
    "bk_commit_points_stats": "bk_ctx *ctx, int64_t out[4]",
}


@pytest.mark.parametrize("name", list(PROTOS))
def test_prototypes_and_bindings(name):
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    assert len(_lib.ALL_KERNELS) == 21
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name
    assert re.sub(r"\s+", " ", m.group(1)).strip() == PROTOS[name]
    assert hasattr(L, name)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args[0] is ctypes.c_void_p
    assert len(args) == PROTOS[name].count(",") + 1


# The checks behind the context never dereference the handle before they have
# passed, so a context that was never created stands in for one (fake).
class _Ctx(ctypes.Structure):
    _fields_ = [("pad", ctypes.c_char * 1)]


_KEEP = _Ctx()
_PT = np.full((3 * 6 + 1, 64), 7, dtype=np.uint8)
_SLOTS = np.zeros(4, dtype=np.int64)
_N = ctypes.c_int64(-5)
_ST = (ctypes.c_int64 * 4)(9, 9, 9, 9)


def _calls(ctx):
    """name -> a call with valid arguments apart from the overrides."""
    L, H = _lib.lib(), _lib.BK_HOST
    pp, sp = _PT.ctypes.data, _SLOTS.ctypes.data
    return {
        "begin": lambda chunks=3, held=5, n_cap=8: L.bk_commit_points_begin(ctx, chunks, held, n_cap),
        "add": lambda c=pp, k=pp, w=pp, where=H: L.bk_commit_points_add(ctx, c, k, w, where,
                                                                        ctypes.byref(_N)),
        "count": lambda n=ctypes.byref(_N): L.bk_commit_points_count(ctx, n),
        "lanes": lambda lanes=0: L.bk_commit_points_set_lanes(ctx, lanes),
        "sum": lambda s=sp, count=4, where=H, c=pp, k=pp, w=pp: L.bk_commit_points_sum(
            ctx, s, count, where, c, k, w),
        "stats": lambda out=_ST: L.bk_commit_points_stats(ctx, out),
    }


CASES = [(e, {}, "null context", True) for e in ("begin", "add", "count", "lanes", "sum", "stats")] + [
    ("sum", dict(s=None, count=0, where=9, c=None, k=None, w=None), "null context", True),
    ("begin", dict(chunks=0), "chunks=0", False),
    ("begin", dict(held=0), "held=0", False),
    ("begin", dict(held=65), "held=65", False),
    ("begin", dict(n_cap=0), "n_cap=0", False),
    ("begin", dict(n_cap=4097), "n_cap=4097", False),
    ("lanes", dict(lanes=3), "lanes=3", False),
    ("lanes", dict(lanes=32), "lanes=32", False),
    ("add", dict(where=3), "where=3", False),
    ("add", dict(c=None), "null commit64", False),
    ("add", dict(k=None), "null chunk_pts", False),
    ("add", dict(w=None), "null witness_pts", False),
    ("count", dict(n=None), "null count", False),
    ("sum", dict(s=None), "null slots", False),
    ("sum", dict(count=0), "count=0", False),
    ("sum", dict(where=3), "where=3", False),
    ("sum", dict(c=None, k=None, w=None), "no output", False),
    ("stats", dict(out=None), "null out", False),
]


@pytest.mark.parametrize("entry,kw,word,null_ctx", CASES)
def test_refusals_need_no_state(entry, kw, word, null_ctx):
    L = _lib.lib()
    call = _calls(None if null_ctx else ctypes.addressof(_KEEP))[entry]
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call(**kw) == _lib.BK_EINVAL
    msg = _lib.last_error()
    assert msg != before and word in msg, (word, msg)
    assert _N.value == -5 and list(_ST) == [9, 9, 9, 9] and (_PT == 7).all()


def _engine():
    """An Engine whose context is never made: the wrappers must refuse first."""
    from biscotti_amd.krum import Engine
    e = object.__new__(Engine)
    e._ctx = None
    return e


Z = np.zeros
WRAPPER_CASES = {
    "begin chunks": lambda e: e.commit_points_begin(0, 5, 8),
    "begin held": lambda e: e.commit_points_begin(3, 65, 8),
    "begin n_cap": lambda e: e.commit_points_begin(3, 5, 4097),
    "lanes": lambda e: e.commit_points_set_lanes(3),
    "add before begin": lambda e: e.commit_points_add(bytes(64), Z((3, 64), np.uint8), Z((3, 5, 64), np.uint8)),
    "sum before begin": lambda e: e.commit_points_sum([0]),
    "commit length": lambda e: _begun(e).commit_points_add(bytes(63), Z((3, 64), np.uint8), Z((3, 5, 64), np.uint8)),
    "chunk count": lambda e: _begun(e).commit_points_add(bytes(64), Z((4, 64), np.uint8), Z((3, 5, 64), np.uint8)),
    "chunk dtype": lambda e: _begun(e).commit_points_add(bytes(64), Z((3, 64), np.int8), Z((3, 5, 64), np.uint8)),
    "witness count": lambda e: _begun(e).commit_points_add(bytes(64), Z((3, 64), np.uint8), Z((3, 4, 64), np.uint8)),
    "witness last axis": lambda e: _begun(e).commit_points_add(bytes(64), Z((3, 64), np.uint8), Z((3, 10, 32), np.uint8)),
    "slots empty": lambda e: _begun(e).commit_points_sum([]),
    "slots float": lambda e: _begun(e).commit_points_sum(np.zeros(2)),
    "no output": lambda e: _begun(e).commit_points_sum([0], False, False, False),
}


def _begun(e):
    e._points = (3, 5)
    return e


@pytest.mark.parametrize("case", list(WRAPPER_CASES))
def test_wrappers_validate_before_the_library(case):
    with pytest.raises(ValueError) as ei:
        WRAPPER_CASES[case](_engine())
    assert "null context" not in str(ei.value)


def test_sources_module_surface_and_go_shim():
    for s in ("bk_commit_points.hip", "bk_commit_points_api.hip", "bk_commit_dev.h"):
        assert os.path.exists(os.path.join(build.CSRC, s)) and (s in build.SOURCES or s.endswith(".h"))
    from biscotti_amd import commit
    assert "PointStore" in commit.__all__
    assert callable(commit.PointStore.add_part) and callable(commit.PointStore.miner_points)
    import go_shim_check as G
    go = open(G.SHIM).read()
    assert {"beginPointsGPU", "addMinerPointsGPU", "getMinerPointsGPU"} <= \
        {name for name, _, _ in G._functions(go)}
    assert {"bk_commit_points_begin", "bk_commit_points_add", "bk_commit_points_sum"} <= \
        {name for name, _, _ in G.shim_calls(go)}
    assert G.check_names(go, open(G.HEADER).read()) == []
    ok, diag, _ = G.compile_check(go, os.path.dirname(G.HEADER))
    assert ok, diag
