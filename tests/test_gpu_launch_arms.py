"""Every arm of the general chain's launch dispatch (bk_gram.hip launch_gram,
bk_mean.hip launch_k4), through bk_multikrum_device and bk_aggregate_device on
an MI355X, against the CPU oracle.

The launchers pick a kernel from the dtype, the leading dimension and the base
address of the rows.  Each case below leaves the launcher one choice:

  fp64  ld 70, aligned base   K1 v3, k_mean<double, VEC>
  fp64  ld 71                 K1 v1 scalar loads, k_mean<double, scalar>
  fp64  ld 70, base + 1       the same two (8-byte aligned rows only)
  fp32  ld 72                 K1 v3, k_mean_f4
  fp32  ld 70                 K1 v1 pair loads, k_mean<float, VEC>
  fp32  ld 71                 K1 v1 scalar loads, k_mean<float, scalar>

n = 130 is above the one-launch path (n <= 128), so K1, K1b, K2, K3, K3b and K4
run as separate kernels; d = 70 is no multiple of a k-block or of a column
quad.  The SEG cases select m = 1,040 >= MEAN_SEG_MIN rows; the ACCUM cases are
bk_aggregate_device at the aligned and the odd ld.  Which kernel ran is not
asserted (the product has no hook for it).

The rows are written by bk_synth_fill_device, which is bitwise the oracle's
generator (test_gpu_parity.py test_gpu_generator_matches_cpu); the tolerances
are test_gpu_parity.py's: selection equal, scores within 1e-9 of the largest
score, mean within 1e-9 of the norm-wise scale.  The selection margin must not
report a near tie, so no comparison is excused by one.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

D = 70
SEED = 20261020


@functools.lru_cache(maxsize=None)
def _reference(n, f, fp32):
    """The oracle's batch and its Multi-Krum, once per (n, f, dtype); read-only."""
    from oracle import oracle as O
    X = O.synth(n, D, SEED + n, f, dtype=np.float32 if fp32 else np.float64)
    sel, sc, mean = O.krum(X, f)
    for a in (X, sel, sc, mean):
        a.setflags(write=False)
    return X, sel, sc, mean


def _device_rows(engine, n, f, fp32, ld, off):
    """n x D rows of the reference batch in a torch buffer: row i starts at
    element off + i * ld.  The padding stays zero."""
    buf = torch.zeros(off + n * ld, dtype=torch.float32 if fp32 else torch.float64, device="cuda")
    rows = buf[off:]
    assert rows.data_ptr() % 16 == (off * buf.element_size()) % 16
    engine.synth_fill_ptr(rows.data_ptr(), _lib.BK_F32 if fp32 else _lib.BK_F64, n, D, ld, 0, D,
                          SEED + n, f)
    return buf, rows


def _check_multikrum(engine, n, f, fp32, ld, off):
    X, osel, osc, omean = _reference(n, f, fp32)
    buf, rows = _device_rows(engine, n, f, fp32, ld, off)
    sel = torch.empty(n - f, dtype=torch.int64, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    mean = torch.empty(D, dtype=torch.float64, device="cuda")
    engine.multikrum_device_ptr(rows.data_ptr(), _lib.BK_F32 if fp32 else _lib.BK_F64, n, D, ld, f,
                                sel.data_ptr(), sc.data_ptr(), mean.data_ptr())
    engine.synchronize()
    mg = engine.selection_margin()
    sel, sc, mean = sel.cpu().numpy(), sc.cpu().numpy(), mean.cpu().numpy()
    print("n %d f %d %s ld %d off %d: gap %.4g err_bound %.4g" %
          (n, f, "fp32" if fp32 else "fp64", ld, off, mg["gap"], mg["err_bound"]))
    assert mg["near_tie"] is False, mg
    assert np.array_equal(sel, osel)
    assert np.max(np.abs(sc - osc)) <= 1e-9 * max(1e-300, np.max(np.abs(osc)))
    mscale = np.max(np.mean(np.abs(X[osel].astype(np.float64)), axis=0))
    assert np.max(np.abs(mean - omean)) <= 1e-9 * mscale


@pytest.mark.parametrize("fp32,ld,off", [
    (False, 70, 0),   # v3 Gram, vector mean
    (False, 71, 0),   # K1 v1 and scalar mean
    (False, 70, 1),   # K1 v1 and scalar mean: the base is 8-byte aligned only
    (True, 72, 0),    # v3 Gram, k_mean_f4
    (True, 70, 0),    # K1 v1, pair mean
    (True, 71, 0),    # scalar mean
])
def test_multikrum_arm(engine, fp32, ld, off):
    _check_multikrum(engine, 130, 40, fp32, ld, off)


@pytest.mark.parametrize("fp32", [False, True])
def test_segmented_mean_arm(engine, fp32):
    """m = 1,040 selected rows: K4 in segments of MEAN_SEG_ROWS, then k_mean_comb."""
    _check_multikrum(engine, 1100, 60, fp32, D, 0)


@pytest.mark.parametrize("fp32,ld", [(False, 70), (False, 71), (True, 72), (True, 71)])
def test_accumulate_arm(engine, oracle, fp32, ld):
    """bk_aggregate_device (K4's ACCUM variant) against aggregate_oracle, bit for bit."""
    n, f, m = 130, 40, 77
    X = _reference(n, f, fp32)[0]
    rng = np.random.default_rng(ld + 2 * fp32)
    idx = rng.integers(0, n, size=m).astype(np.int64)  # any order, duplicates allowed
    g0 = rng.standard_normal(D)
    want = oracle.aggregate(X.astype(np.float64), idx, g0)
    buf, rows = _device_rows(engine, n, f, fp32, ld, 0)
    tI, tG = torch.from_numpy(idx).cuda(), torch.from_numpy(g0.copy()).cuda()
    engine.aggregate_device_ptr(rows.data_ptr(), _lib.BK_F32 if fp32 else _lib.BK_F64, n, D, ld,
                                tI.data_ptr(), m, tG.data_ptr())
    engine.synchronize()
    assert np.array_equal(tG.cpu().numpy().view(np.int64), want.view(np.int64))
