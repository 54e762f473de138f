"""MI355X: K1's glds split (which wave issues which global_load_lds of a stage,
and where in its MFMA stream) must not move a bit.

The split changes neither an MFMA nor the order of any Gram element's sum, so
the packed upper triangle from `bk_gram_upper_device` and the selection, scores
and mean of the full call equal, bit for bit, what the library of the commit
before the change wrote for the same inputs (tests/golden/glds_*.npz, recorded
once by tests/golden/gen_glds_split_goldens.py).  A glds issued into a stage
that is still being read, or a vmcnt wait that counts the wrong wave class's
loads, shows here as wrong bits: the shapes cover both group kinds (NB = 4 and
6) over a ring that wraps many times, a lone super-block, an odd super-block
count, three k-blocks and one (the prologue alone fills the ring), widened
fp32 rows, and the fp32-MFMA instance, which keeps its even split.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gen_glds_split_goldens as GG  # noqa: E402
import golden_util as GU  # noqa: E402


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r != %r" % (
        what, bad.size, g.size, bad[0], got.flat[bad[0]], want.flat[bad[0]])


@pytest.mark.parametrize("name", list(GG.CASES))
def test_bits_equal_the_parent_library(engine, name):
    g = GU.load(name)
    assert GG.digest(GG.rows(name)) == str(g["input_sha256"]), "the input itself differs"
    U, sel, sc, mean = GG.run(engine, name)
    if "upper" in g.files:
        _same_bits(U, g["upper"], "packed upper")
    else:
        _same_bits(U[::GG.SAMPLE].copy(), g["upper_sample"], "packed upper (every %dth)" % GG.SAMPLE)
    assert GG.digest(U) == str(g["upper_sha256"]), "packed upper: SHA-256 differs"
    assert np.array_equal(sel, g["sel"]), "selection"
    _same_bits(sc, g["scores"], "scores")
    _same_bits(mean, g["mean"], "mean")
