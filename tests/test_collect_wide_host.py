"""The host side of the wide collection finishes, without a GPU: the queue map
of k_collect_wide_ragged (bk_ragged_queue_item with the wide item counts, the
function the kernel and the host entry both decode with) against a model built
position by position, and the additive entry bk_set_collect_wide in the header,
the binding and the built library under an unchanged BK_ABI_VERSION."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from biscotti_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 2048  # columns per wide M item
WIDE_MAX_D = 1 << 20


def _model(ns, C):
    """S_0 | S_1 M_0 | S_2 M_1 | ... | S_{W-1} M_{W-2} | M_{W-1}: (problem, item)
    per queue position; problem p's M item c is its item n_p + c"""
    q = [(0, it) for it in range(ns[0])]
    for j in range(1, len(ns)):
        q += [(j, it) for it in range(ns[j])]
        q += [(j - 1, ns[j - 1] + c) for c in range(C)]
    q += [(len(ns) - 1, ns[-1] + c) for c in range(C)]
    return q


def _decode(ns, C, item):
    arr = (ctypes.c_int32 * len(ns))(*ns)
    p, it = ctypes.c_int(-1), ctypes.c_int(-1)
    st = _lib.lib().bk_ragged_queue_item(arr, len(ns), C, item, ctypes.byref(p), ctypes.byref(it))
    return st, p.value, it.value


C_LO, C_HI = -(-32769 // W), -(-WIDE_MAX_D // W)


@pytest.mark.parametrize("C", sorted({C_LO, C_LO + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                                      C_HI - 1, C_HI}))
@pytest.mark.parametrize("ns", [(113, 128, 120, 127, 113), (1, 16, 2, 9, 16, 3), (100,), (97, 112)])
def test_queue_map_at_wide_item_counts(ns, C):
    """every position of the queue, for the item counts of 32,769 <= d <= 2^20
    (17 .. 512) and mixed n within one NB group"""
    assert (C_LO, C_HI) == (17, 512)
    model = _model(list(ns), C)
    assert len(model) == sum(ns) + len(ns) * C
    for item, want in enumerate(model):
        st, p, it = _decode(ns, C, item)
        assert st == 0 and (p, it) == want, (ns, C, item, (p, it), want)
    assert _decode(ns, C, len(model))[0] == _lib.BK_EINVAL
    assert _decode(ns, C, -1)[0] == _lib.BK_EINVAL


def test_queue_map_random_mixed():
    rng = np.random.default_rng(12)
    for _ in range(20):
        Wp = int(rng.integers(1, 9))
        ns = [int(v) for v in rng.integers(1, 129, size=Wp)]
        C = int(rng.integers(C_LO, C_HI + 1))
        model = _model(ns, C)
        for item in rng.choice(len(model), size=min(400, len(model)), replace=False):
            st, p, it = _decode(ns, C, int(item))
            assert st == 0 and (p, it) == model[int(item)], (ns, C, item)


def test_the_entry_is_additive():
    src = open(os.path.join(REPO, "include", "bk.h")).read()
    assert re.search(r"^int bk_set_collect_wide\(bk_ctx \*ctx, int on\);", src, flags=re.M)
    assert re.search(r"^#define BK_COLLECT_WIDE_MAX_D 1048576$", src, flags=re.M)
    # with a mean the wide launch stops at a whole number of 2,048-column items
    mm = re.search(r"^#define BK_COLLECT_WIDE_MEAN_MAX_D (\d+)\b", src, flags=re.M)
    assert mm and 32768 < int(mm.group(1)) <= WIDE_MAX_D and int(mm.group(1)) % W == 0
    assert re.search(r"^#define BK_ABI_VERSION 14$", src, flags=re.M)
    assert _lib.SIGNATURES["bk_set_collect_wide"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    L = _lib.lib()
    assert hasattr(L, "bk_set_collect_wide")
    assert L.bk_abi_version() == _lib.BK_ABI_VERSION == 14
    assert len(_lib.KERNELS) == 19  # the wide launches are timed under k_small
    assert L.bk_set_collect_wide(None, 1) == _lib.BK_EINVAL and _lib.last_error()


def test_python_surface():
    from biscotti_amd.krum import Engine, KRUMValidator
    assert inspect.signature(Engine.set_collect_wide).parameters["on"].default is True
    assert inspect.signature(KRUMValidator.__init__).parameters["wide"].default is False
