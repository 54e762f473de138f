"""bk_set_collect_wide_arrive and k_collect_arrive_wide's queue without a GPU:
the prototypes in include/bk.h, the bindings in the built library, the unchanged
ABI version, the argument checks that need no context, and the item numbering
(bk_collect_wide_arrive_item) over EVERY item of four launches: each (chunk,
row) unit of the border in exactly one B item, each Gram element of the new run
in exactly one R item, the kinds in the order B < R < S < M, and the counts the
launcher takes from the same function."""
import ctypes
import os
import re

import pytest

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, R, S, M = 0, 1, 2, 3
CHUNK_BYTES = 8192  # of a row per border chunk (bk_internal.h COLLECT_BORDER_CHUNK_BYTES)
WAVES = 8           # of a workgroup: rows of a B item per round, elements of an R item
MAX_B = 1024        # B items the queue lines count (32 groups of 32)
WIDE_COLS = 2048    # columns per wide mean item


def _proto(name):
    """the C prototype of `name` in include/bk.h, comments dropped, white space collapsed"""
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_prototypes_and_bindings():
    L = _lib.lib()
    assert L.bk_abi_version() == 14 == _lib.BK_ABI_VERSION
    with open(os.path.join(REPO, "include", "bk.h")) as fh:
        text = fh.read()
    assert re.search(r"#define\s+BK_ABI_VERSION\s+14\b", text)
    assert _proto("bk_set_collect_wide_arrive") == "bk_ctx *ctx, int on"
    assert _proto("bk_collect_wide_arrive_item") == (
        "int64_t rows, int64_t d, int dtype, int64_t n, int mean, int64_t item, int *kind, "
        "int *a, int *b, int64_t counts[4]")
    assert _proto("bk_set_collect_wide") == "bk_ctx *ctx, int on"
    assert _proto("bk_collect_stats") == "bk_ctx *ctx, int64_t out[4]"
    i, p = ctypes.c_int, ctypes.c_void_p
    for name in ("bk_set_collect_wide_arrive", "bk_collect_wide_arrive_item"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["bk_set_collect_wide_arrive"]
    assert res is i and args == [p, i]


def _fresh_message(call, status, word):
    L = _lib.lib()
    # another entry's message first, so the one read below is this call's
    assert L.bk_check_args(0, 0, 0) == _lib.BK_EINVAL
    before = _lib.last_error()
    assert call() == status
    msg = _lib.last_error()
    assert msg and msg != before and word in msg, msg


def test_null_context_is_einval():
    L = _lib.lib()
    _fresh_message(lambda: L.bk_set_collect_wide_arrive(None, 1), _lib.BK_EINVAL, "null context")
    _fresh_message(lambda: L.bk_set_collect_wide_arrive(None, 0), _lib.BK_EINVAL, "null context")


def test_engine_and_validator_surface():
    from biscotti_amd.krum import Engine, KRUMValidator
    assert callable(Engine.set_collect_wide_arrive)
    v = KRUMValidator(collect=True, wide=True, wide_arrive=True)
    assert v._wide_arrive and not KRUMValidator(collect=True, wide=True)._wide_arrive
    for kw in ({"wide_arrive": True}, {"collect": True, "wide_arrive": True}):
        with pytest.raises(ValueError, match="wide=True"):
            KRUMValidator(**kw)


def _item(rows, d, dtype, n, mean, item):
    kind, a, b = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    counts = (ctypes.c_int64 * 4)()
    st = _lib.lib().bk_collect_wide_arrive_item(rows, d, dtype, n, mean, item, ctypes.byref(kind),
                                                ctypes.byref(a), ctypes.byref(b), counts)
    return st, kind.value, a.value, b.value, list(counts)


def _expected_counts(rows, d, dtype, n, mean):
    """the layout from its description, not from the library"""
    es = 8 if dtype == _lib.BK_F64 else 4
    chunks = -(-d * es // CHUNK_BYTES)
    rpb = WAVES
    while chunks * -(-rows // rpb) > MAX_B:
        rpb += WAVES
    return chunks, rpb, [chunks * -(-rows // rpb), -(-rows // WAVES), n, -(-d // WIDE_COLS) if mean else 1]


@pytest.mark.parametrize("rows,d,dtype", [(2, 32769, _lib.BK_F64), (17, 66001, _lib.BK_F64),
                                          (100, 163850, _lib.BK_F32),
                                          (128, 1048576, _lib.BK_F64)])
@pytest.mark.parametrize("mean", [0, 1])
def test_every_item(rows, d, dtype, mean):
    n = rows
    chunks, rpb, want = _expected_counts(rows, d, dtype, n, mean)
    total = sum(want)
    assert want[0] <= MAX_B
    covered = {}   # (chunk, row) -> B items that cover it
    elements = {}  # Gram element i of the new run -> R items that cover it
    rows_s, items_m, kinds = [], [], []
    for it in range(total):
        st, kind, a, b, counts = _item(rows, d, dtype, n, mean, it)
        assert st == _lib.BK_OK, (it, _lib.last_error())
        assert counts == want, (it, counts, want)
        kinds.append(kind)
        if kind == B:
            assert 0 <= a < chunks and 0 <= b * rpb < rows, (it, a, b)
            for i in range(b * rpb, min(rows, (b + 1) * rpb)):
                covered[(a, i)] = covered.get((a, i), 0) + 1
        elif kind == R:
            assert a % WAVES == 0 and 1 <= b <= WAVES and a + b <= rows, (it, a, b)
            for i in range(a, a + b):
                elements[i] = elements.get(i, 0) + 1
        elif kind == S:
            rows_s.append(a)
        else:
            assert kind == M
            items_m.append(a)
    # every (chunk, row i <= j) unit exactly once, every element i <= j exactly once
    assert covered == {(s, i): 1 for s in range(chunks) for i in range(rows)}
    assert elements == {i: 1 for i in range(rows)}
    assert rows_s == list(range(n)) and items_m == list(range(want[3]))
    # B < R < S < M, each kind's count what the launcher passes
    assert kinds == sorted(kinds)
    assert [kinds.count(k) for k in (B, R, S, M)] == want
    # the ends of the queue
    for it in (-1, total):
        st = _item(rows, d, dtype, n, mean, it)[0]
        assert st == _lib.BK_EINVAL and "outside the queue" in _lib.last_error()


def test_layout_refusals():
    for rows, d, dtype, n in ((0, 40000, 0, 2), (129, 40000, 0, 2), (5, 40000, 2, 2),
                              (5, 40000, 0, 129), (5, 0, 0, 2), (5, 1048577, 0, 2)):
        st = _item(rows, d, dtype, n, 0, 0)[0]
        assert st == _lib.BK_EINVAL and "need 1 <= rows" in _lib.last_error(), (rows, d, dtype, n)
    L = _lib.lib()
    assert L.bk_collect_wide_arrive_item(5, 40000, 0, 5, 0, 0, None, None, None, None) == _lib.BK_EINVAL
    assert "null kind" in _lib.last_error()
