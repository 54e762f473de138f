"""MI355X: scores and near-tie flags of every path that produces scores, against
the exact double-double reference (tests/exact_ref.py).

include/bk.h bk_selection_margin claims that every score computed here lies
within e_here of the exact one, so that near_tie = 0 proves the reference selects
exactly sel_idx.  The other tests compare the record with its own formula, and
scores with fp64 evaluations at 1e-9 of the largest score; none compares a score
with an exact score.  Per case (tests/exact_cases.py: the path is in the id) a
ladder of inputs moves the boundary gap through the call's err_bound, and on
every rung:

1. the record is understood: margin_bound(M, d, k, u_G, e_G) reproduces err_bound
   to 1e-12, u_G and e_G read from a bk_gram_upper_device call on the same rows in
   the same mode, and M >= exact M (1 - 2 gamma_{d+2}(u_G)) - e_G;
2. every score is within e_here of the exact score;
3. near_tie = 0 implies sel = the exact selection;
4. an exact gap above err_bound + 2 e_here is not flagged;
5. the exact tie is flagged and goes to the lower index;
and each ladder holds at least two flagged and two unflagged rungs.  A certified
sibling mode returns the exact selection on every rung with a nonzero gap.

The exact-arithmetic paths (u_G = 2^-53, no int8 term) also pass a sharper gate,
K x max(the CPU oracle's error on the same input, 4 ulp of the largest exact
score): K = SHARP_K below, measured against the oracle on the MI355X
(tools/exact_scores_report.py, profiles/r20/exact_scores.json).

test_gram_entries localises a failure: the packed Gram of every mode, entry by
entry, within gamma_{d+2}(u_G) sqrt(G*_ii G*_jj) + e_G of the exact Gram (Cauchy-
Schwarz on the standard dot-product bound).

The general chain at n = 130 is one workgroup group whatever d is (bk_plan's S
counts sets of row blocks: three blocks fit one set), so the split-K case asserts
what makes it one: more 16-column k-blocks than K1 has workgroups; the two large-n
cases assert S > 1.
"""
import numpy as np
import pytest

import exact_cases as EC
import golden_util as GU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from biscotti_amd import _lib  # noqa: E402

# The sharper gate's factor: the next power of two at or above 4x the largest
# ratio (GPU error) / max(oracle error, 4 ulp) over the exact-path cases, as
# measured on an MI355X (profiles/r20/exact_scores.json: the largest ratio is 1.00,
# k_small on fp32 rows at 128 x 70).  Every case's e_here / max(oracle error,
# 4 ulp) is at least 22, so the gate binds everywhere; a rung where it would not
# is skipped (run_case).
SHARP_K = 4.0


def _dt(case):
    return _lib.BK_F32 if case["dtype"] == np.float32 else _lib.BK_F64


def _set_mode(engine, case, name):
    mode = getattr(_lib, name) if name else 0
    (engine.set_f32_mode if case["dtype"] == np.float32 else engine.set_f64_mode)(mode)


def _to_device(case, X):
    """The rows at the case's leading dimension, the padding NaN (never read)."""
    n, d = X.shape
    buf = torch.full((n, case["ld"]), float("nan"), device="cuda",
                     dtype=torch.float32 if case["dtype"] == np.float32 else torch.float64)
    buf[:, :d] = torch.tensor(X).cuda()  # a copy: the shared inputs are read-only
    return buf


def _record(engine, case, buf, n, d):
    """(u_G, e_G) from the trailing record of bk_gram_upper_device on the same rows."""
    U = torch.empty(int(_lib.lib().bk_upper_elems(n)), dtype=torch.float64, device="cuda")
    engine.gram_upper_ptr(buf.data_ptr(), _dt(case), n, d, case["ld"], U.data_ptr())
    engine.synchronize()
    U = U.cpu().numpy()
    assert U[-4] == d
    return U, (2.0 ** -24 if U[-3] > 0 else 2.0 ** -53), float(U[-2])


def _device_call(engine, case, buf, n, d, f):
    sel = torch.empty(n - f, dtype=torch.int64, device="cuda")
    sc = torch.empty(n, dtype=torch.float64, device="cuda")
    mean = torch.empty(d, dtype=torch.float64, device="cuda")
    engine.multikrum_device_ptr(buf.data_ptr(), _dt(case), n, d, case["ld"], f, sel.data_ptr(),
                                sc.data_ptr(), mean.data_ptr())
    engine.synchronize()
    return sel.cpu().numpy(), sc.cpu().numpy()


def _collect_call(engine, case, X, f):
    """Shuffled arrival in groups of 1, 7 and the rest; the finish in sorted order."""
    n, d = X.shape
    perm = np.random.default_rng(n + d).permutation(n)
    engine.collect_begin(n, d, case["dtype"])
    engine.collect_add(X[perm[0]])
    engine.collect_add([X[i] for i in perm[1:8]])
    engine.collect_add([X[i] for i in perm[8:]])
    slot = np.empty(n, dtype=np.int64)
    slot[perm] = np.arange(n)
    sel, sc, _ = engine.collect_finish(order=slot, n=n, f=f)
    return sel, sc


def run_case(engine, oracle, case, sharp_k=None):
    """Every rung of a case through its path; the assertions of the module's
    docstring; the figures tools/exact_scores_report.py records."""
    n, d, f = case["n"], case["d"], case["f"]
    k, pair = n - f - 2, EC.ladder_pair(n)
    plan = engine.plan(n, d)
    if "splitK" in case["id"]:
        assert plan["S"] == 1 and -(-d // plan["kc"]) > plan["nwg"]
    if n > 1024:
        assert plan["S"] > 1
    fig = dict(id=case["id"], n=n, d=d, f=f, rungs=[], flagged=0, unflagged=0)
    for t, X, ex in EC.rung_inputs(case):
        buf = _to_device(case, X)
        try:
            if case["entry"] == "collect":
                U, u_gram, eg = _record(engine, case, buf, n, d)
                sel, sc = _collect_call(engine, case, X, f)
            else:
                _set_mode(engine, case, case["mode"])
                U, u_gram, eg = _record(engine, case, buf, n, d)
                sel, sc = _device_call(engine, case, buf, n, d, f)
            mg = engine.selection_margin()
            assert u_gram == case["u_gram"] and (eg > 0.0) == case["int8"], (u_gram, eg)
            # 1. the record
            assert mg["d"] == d and mg["k"] == k
            want = GU.margin_bound(mg["M"], d, k, u_gram, eg)
            assert abs(mg["err_bound"] - want) <= 1e-12 * want, (mg["err_bound"], want)
            assert mg["near_tie"] == (not mg["gap"] > mg["err_bound"])
            assert mg["M"] >= ex.M * (1.0 - 2.0 * GU.gamma(d + 2.0, u_gram)) - eg
            e_here, _ = GU.margin_e(mg["M"], d, k, u_gram, eg)
            # 2. - 5.
            err = float(np.max(np.abs(sc - ex.scores)))
            _, osc, _ = oracle.krum(X, f, want_mean=False)
            oerr = float(np.max(np.abs(osc - ex.scores)))
            floor = max(oerr, 4.0 * float(np.spacing(np.max(ex.scores))))
            fig["rungs"].append(dict(t=t, gap=ex.gap, err_bound=mg["err_bound"], e_here=e_here,
                                     gpu_err=err, oracle_err=oerr, floor=floor,
                                     near_tie=bool(mg["near_tie"])))
            EC.check_rung(ex, sel, sc, mg["near_tie"], mg["err_bound"], e_here, pair=pair,
                          tie=t is None)
            if EC.exact_path(case) and sharp_k is not None and sharp_k < e_here / floor:
                assert err <= sharp_k * floor, (case["id"], t, err, oerr, sharp_k)
            if t is not None:
                fig["flagged"] += bool(mg["near_tie"])
                fig["unflagged"] += not mg["near_tie"]
            if case["cert"]:
                _set_mode(engine, case, case["cert"])
                sel2, _ = _device_call(engine, case, buf, n, d, f)
                if ex.gap > 0.0:
                    assert np.array_equal(sel2, ex.sel), (case["cert"], t)
        finally:
            _set_mode(engine, case, None)
    r = fig["rungs"]
    fig["gpu_err"] = max(x["gpu_err"] for x in r)
    fig["oracle_err"] = max(x["oracle_err"] for x in r)
    fig["e_here"] = min(x["e_here"] for x in r)
    fig["err_over_e_here"] = max(x["gpu_err"] / x["e_here"] for x in r)
    fig["err_over_floor"] = max(x["gpu_err"] / x["floor"] for x in r)
    fig["e_here_over_floor"] = min(x["e_here"] / x["floor"] for x in r)
    fig["sharp_gate"] = bool(EC.exact_path(case) and sharp_k is not None
                             and sharp_k < fig["e_here_over_floor"])
    # no ladder passes vacuously
    assert fig["flagged"] >= 2 and fig["unflagged"] >= 2, fig
    return fig


@pytest.mark.parametrize("cid", EC.CASE_IDS)
def test_scores_and_flags_against_exact(cid, engine, oracle):
    case = EC.CASES[EC.CASE_IDS.index(cid)]
    fig = run_case(engine, oracle, case, SHARP_K)
    print("%s: max |s - s*| %.3e (oracle %.3e), e_here %.3e, error / e_here %.2e, error / "
          "max(oracle, 4 ulp) %.2f, %d unflagged and %d flagged rungs, sharp gate %s"
          % (cid, fig["gpu_err"], fig["oracle_err"], fig["e_here"], fig["err_over_e_here"],
             fig["err_over_floor"], fig["unflagged"], fig["flagged"],
             "on" if fig["sharp_gate"] else "off"))


GRAM_CASES = ["chain-f64-ld70-K1v3", "chain-f64-ld71-K1v1", "chain-f32-ld72-K1v3",
              "chain-f32-ld70-K1v1", "mode-f32-MFMA", "mode-f32-I8", "mode-f32-I8X2",
              "mode-f64-I8", "mode-f64-I8X2"]


@pytest.mark.parametrize("cid", GRAM_CASES)
def test_gram_entries(cid, engine):
    """bk_gram_upper_device in every mode at 130 x 70 / 130 x 72, entry by entry
    against the double-double Gram: where a score failure comes from (K1, K1i8 or
    the finish)."""
    from biscotti_amd.dist import unpack_upper
    case = EC.CASES[EC.CASE_IDS.index(cid)]
    n, d = case["n"], case["d"]
    t, X, ex = EC.rung_inputs(case)[0]
    buf = _to_device(case, X)
    try:
        _set_mode(engine, case, case["mode"])
        U, u_gram, eg = _record(engine, case, buf, n, d)
    finally:
        _set_mode(engine, case, None)
    assert u_gram == case["u_gram"] and (eg > 0.0) == case["int8"]
    G = unpack_upper(U, n)
    dg = np.diagonal(ex.Gh)
    bound = GU.gamma(d + 2.0, u_gram) * np.sqrt(dg[:, None] * dg[None, :]) + eg
    err = np.abs((G - ex.Gh) - ex.Gl)
    print("%s: max |G - G*| %.3e, max of error / bound %.3e, e_G %.3e"
          % (cid, float(err.max()), float((err / bound).max()), eg))
    assert np.all(err <= bound)
