"""CPU: the share arithmetic's reference forms against each other
(tests/shares_ref.py): the Horner form of createShareAndWitness's value against
the literal one, the exact recovery against the wrapping sum of the quantised
deltas, and the reference's float recovery against the exact one."""
import random

import numpy as np
import pytest

import shares_ref as R

P, T, PREC = 10, 20, 4
PARTIAL = list(range(0, 5)) + list(range(10, 16))  # one of four miners missing


def _coef_cases():
    rng = random.Random(2501)
    cases = [[0], [7], [-1], [1 << 62], [-(1 << 62)], [R.INT64_MIN], [(1 << 63) - 1],
             [0] * 10, [5] + [0] * 9, [0] * 9 + [3], [1, 0, 0, 4, 0, 0, 0, 0, 0, 0]]
    for bits in (8, 20, 40, 50, 53, 56, 62):
        for L in (1, 2, 5, 9, 10):
            cases.append([rng.randint(-(1 << bits), 1 << bits) for _ in range(L)])
    # zeros in the leading places, large below
    cases.append([rng.randint(-(1 << 62), 1 << 62) for _ in range(6)] + [0] * 4)
    cases.append([rng.randint(-(1 << 50), 1 << 50) for _ in range(3)] + [0, 0, 1 << 50, 0])
    return cases


def test_horner_form_is_the_literal_one():
    n = 0
    for coefs in _coef_cases():
        for s in list(range(0, 24)) + [40, 63]:  # s = 10 is x = 0
            assert R.share_value_horner(coefs, s) == R.share_value_literal(coefs, s), (coefs, s)
            n += 1
    assert n > 1000


def test_small_coefficients_leave_no_correction():
    # every |c_j x^j| < 2^53: the division's remainder is 0 and y is the
    # integer polynomial's value
    rng = random.Random(7)
    for _ in range(50):
        coefs = [rng.randint(-10 ** 6, 10 ** 6) for _ in range(P)]
        for s in range(T):
            x = s - R.X0
            assert R.share_value_horner(coefs, s) == sum(c * x ** j for j, c in enumerate(coefs))


def _summed(n, d, sigma, seed):
    rng = np.random.default_rng(seed)
    deltas = rng.normal(0.0, sigma, size=(n, d))
    shares = R.wrapping_sum([R.generate(dl, PREC, P, T) for dl in deltas])
    qsum = R.wrapping_sum([np.array(R.quantize(dl, PREC), dtype=np.int64) for dl in deltas])
    return shares, qsum


@pytest.mark.parametrize("n,d,sigma", [(1, 25, 0.1), (35, 25, 0.1), (70, 31, 0.1), (20, 10, 100.0)])
def test_exact_recovery_is_the_quantised_sum(n, d, sigma):
    shares, qsum = _summed(n, d, sigma, 100 + n)
    for points in (list(range(T)), PARTIAL):
        xs = [s - R.X0 for s in points]
        got = []
        for c in range(shares.shape[0]):
            m = R.recover_exact(xs, [int(shares[c, s]) for s in points], P)
            assert m is not None
            got += m
        assert got[:d] == qsum.tolist()
        assert all(v == 0 for v in got[d:])


def test_exact_recovery_flags_an_altered_share():
    shares, _ = _summed(5, 10, 0.1, 3)
    xs = [s - R.X0 for s in range(T)]
    ys = [int(v) for v in shares[0]]
    assert R.recover_exact(xs, ys, P) is not None
    for s in (0, 9, 10, 19):  # an interpolation point, and one that only verifies
        bad = list(ys)
        bad[s] += 1
        assert R.recover_exact(xs, bad, P) is None


@pytest.mark.parametrize("n", [1, 5, 35])
def test_float_recovery_agrees_for_small_updates(n):
    shares, qsum = _summed(n, 25, 0.1, 200 + n)
    xs = [s - R.X0 for s in range(T)]
    got = []
    for c in range(shares.shape[0]):
        ys = [int(v) for v in shares[c]]
        rounded, sol = R.recover_float(xs, ys, P)
        # the reference method alone: its solution is near an integer (measured
        # 0.002 at n = 70), well inside the 0.25 cap
        assert np.max(np.abs(sol - np.rint(sol))) < 0.25
        assert rounded.tolist() == R.recover_exact(xs, ys, P)
        got += rounded.tolist()
    assert got[:25] == qsum.tolist()
