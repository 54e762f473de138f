"""CPU: the exact double-double reference (tests/exact_ref.py), and the score and
flag contract of include/bk.h bk_selection_margin with the CPU oracle standing
in for the implementation -- the design of tests/test_gpu_exact_scores.py,
proven before any GPU is involved.

* the double-double Gram against fractions.Fraction arithmetic: 2^-100 of the
  largest entry;
* the oracle (an fp64 evaluation of the reference formula) stays inside e_ref of
  the exact scores on every input the GPU cases use;
* the ladder property: with the flag computed from the oracle's own scores, every
  score is within e_here, near_tie = 0 implies the exact selection, a clear gap
  is not flagged, the exact tie is flagged and goes to the lower index, and each
  ladder holds at least two flagged and two unflagged rungs;
* margin_bound (now written through margin_e) returns the values it returned.
"""
from fractions import Fraction

import numpy as np
import pytest

import exact_cases as EC
import exact_ref as XR
import golden_util as GU


def test_double_double_gram_against_fractions():
    X = EC.cluster(12, 9, 3, 2.0 ** 10, seed=5)
    Gh, Gl = XR.dd_gram(X)
    F = [[Fraction(float(v)) for v in row] for row in X]
    worst, big = Fraction(0), Fraction(0)
    for i in range(12):
        for j in range(12):
            want = sum(F[i][c] * F[j][c] for c in range(9))
            got = Fraction(float(Gh[i, j])) + Fraction(float(Gl[i, j]))
            worst, big = max(worst, abs(got - want)), max(big, abs(want))
    print("double-double Gram: max |G - exact| %.3e on entries up to %.3e"
          % (float(worst), float(big)))
    assert worst <= big * Fraction(1, 2 ** 100)


def test_fp32_rows_widen_exactly():
    X = EC.cluster(12, 9, 3, 2.0 ** 4, seed=6, dtype=np.float32)
    a, b = XR.dd_gram(X), XR.dd_gram(X.astype(np.float64))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_replaced_row_is_bitwise_the_full_gram():
    n, d, f = 70, 33, 20
    X0 = EC.ladder(n, d, f, 2.0 ** 10, None)
    X = EC.ladder(n, d, f, 2.0 ** 10, 8)
    ib = EC.ladder_pair(n)[1]
    assert np.array_equal(np.nonzero((X0 != X).any(axis=1))[0], [ib])
    G = XR.dd_gram_replace_row(XR.dd_gram(X0), X, ib)
    for block in (64, 7):
        W = XR.dd_gram(X, block=block)
        assert np.array_equal(G[0], W[0]) and np.array_equal(G[1], W[1])
    assert np.array_equal(G[0], G[0].T) and np.array_equal(G[1], G[1].T)
    a, b = XR.krum(X, f, gram=G), XR.krum(X, f, block=9)
    assert np.array_equal(a.scores, b.scores) and np.array_equal(a.scores_lo, b.scores_lo)
    assert np.array_equal(a.sel, b.sel) and a.gap == b.gap


def test_exact_selection_on_integers():
    """Small integer rows: every fp64 operation is exact, so plain numpy gives the
    exact scores and the reference must return them bit for bit."""
    rng = np.random.default_rng(3)
    X = rng.integers(-9, 10, size=(21, 13)).astype(np.float64)
    X[7] = X[2]  # a duplicate: an exact tie somewhere in the order
    f = 6
    ex = XR.krum(X, f)
    G = X @ X.T
    D = np.diag(G)[:, None] + np.diag(G)[None, :] - 2.0 * G
    np.fill_diagonal(D, np.inf)
    s = np.sort(D, axis=1)[:, :ex.k].sum(axis=1)
    assert np.array_equal(ex.scores, s) and not ex.scores_lo.any()
    order = np.lexsort((np.arange(21), s))
    assert np.array_equal(ex.order, order)
    assert np.array_equal(ex.sel, np.sort(order[:ex.m]))
    assert ex.gap == s[order[ex.m]] - s[order[ex.m - 1]] and ex.M == np.max(np.diag(G))


PINNED = [
    ((948.3, 70, 88, 2.0 ** -53, 0.0), "0x1.9c90e9999b417p-26"),
    ((854.0, 72, 88, 2.0 ** -24, 0.0), "0x1.536fa67ecad3fp+1"),
    ((854.0, 72, 88, 2.0 ** -53, 0.0162), "0x1.6cf41f2ceffabp+3"),
    ((1370000.0, 262144, 2865, 2.0 ** -24, 0.0), "0x1.ea6c55fc1e3f9p+28"),
    ((216.0, 8, 1468, 2.0 ** -53, 0.0), "0x1.bf8cd00002103p-21"),
    ((3.5, 25, 0, 2.0 ** -53, 0.0), "0x0.0p+0"),
    ((42870.0, 4100, 88, 2.0 ** -53, 1.25), "0x1.b80000ebab4c9p+9"),
]


@pytest.mark.parametrize("args,want", PINNED)
def test_margin_bound_keeps_its_values(args, want):
    """margin_bound before margin_e existed, evaluated on these tuples."""
    assert GU.margin_bound(*args) == float.fromhex(want)
    e_here, e_ref = GU.margin_e(*args)
    assert GU.margin_bound(*args) == 2.0 * (e_here + e_ref) * (1.0 + 2.0 ** -40)
    assert e_here >= e_ref >= 0.0


def _ladder(cid):
    return EC.rung_inputs(EC.CASES[EC.CASE_IDS.index(cid)])


@pytest.mark.parametrize("cid", EC.CASE_IDS)
def test_oracle_stays_inside_e_ref(cid, oracle):
    """The CPU oracle on every input family of the GPU cases: each score within
    e_ref of the exact one (here: 1e-4 .. 2e-2 of it)."""
    case = EC.CASES[EC.CASE_IDS.index(cid)]
    n, d, f = case["n"], case["d"], case["f"]
    inputs = [(t, X, ex) for t, X, ex in _ladder(cid)]
    if n <= 130:
        X = EC.cluster(n, d, f, case["ratio"], dtype=case["dtype"], quiet=case["quiet"])
        inputs.append(("cluster", X, XR.krum(X, f)))
    worst = 0.0
    for t, X, ex in inputs:
        _, osc, _ = oracle.krum(X, f, want_mean=False)
        _, e_ref = GU.margin_e(ex.M, d, ex.k)
        err = float(np.max(np.abs(osc - ex.scores)))
        worst = max(worst, err / e_ref)
        assert err <= e_ref, (cid, t, err, e_ref)
    print("%s: oracle error / e_ref at most %.2e" % (cid, worst))


@pytest.mark.parametrize("cid", [c["id"] for c in EC.CASES if EC.exact_path(c)])
def test_ladder_property_with_the_oracle(cid, oracle):
    """The five assertions of the GPU test, the oracle as the implementation and
    the flag computed from its own scores as write_margin computes it."""
    case = EC.CASES[EC.CASE_IDS.index(cid)]
    n, d, f = case["n"], case["d"], case["f"]
    pair = EC.ladder_pair(n)
    flagged = unflagged = 0
    for t, X, ex in _ladder(cid):
        _, osc, _ = oracle.krum(X, f, want_mean=False)
        M = float(np.max(oracle.sqnorms(X)))
        sel, gap, bound, near, e_here = EC.flag_of(osc, M, d, f)
        assert M >= ex.M * (1.0 - 2.0 * GU.gamma(d + 2.0, 2.0 ** -53))
        EC.check_rung(ex, sel, osc, near, bound, e_here, pair=pair, tie=t is None)
        if t is not None:
            flagged += near
            unflagged += not near
    print("%s: %d unflagged and %d flagged rungs" % (cid, unflagged, flagged))
    assert flagged >= 2 and unflagged >= 2
