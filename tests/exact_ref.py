"""An exact Multi-Krum reference in double-double arithmetic (numpy only).

What the selection margin (include/bk.h bk_selection_margin) promises is stated
against the EXACT scores of the reference formula: every fp64 evaluation lies
within e of them.  The CPU oracle and the numpy goldens are themselves fp64
evaluations, so neither can check that claim; this module can.

Every quantity is an unevaluated sum hi + lo of two doubles (|lo| <= ulp(hi) / 2):
Dekker / Veltkamp two_prod and Knuth two_sum make each product and each sum of
two doubles exact, and the double-double additions that accumulate them lose at
most ~2^-104 of the running magnitude per step.  tests/test_exact_ref.py checks
the Gram against fractions.Fraction arithmetic to 2^-100 of its largest entry.

  Gram        G_ij = sum_c x_ic x_jc, accumulated column by column over (n, n)
              arrays (fp32 rows widened to fp64 first, which is exact).
  distances   G_ii + G_jj - 2 G_ij in double-double; the fp64 matrix returned is
              that value rounded once, the diagonal excluded.
  scores      each row's distances sorted, the k = n - f - 2 smallest summed in
              double-double, rounded once.  The low words of the distances stay
              in the sum, so a score carries one rounding, not k + 1.
  selection   the m = n - f lowest scores under (value, index) order, ascending;
              the order is taken on the double-double scores.
  gap         s*[rank m] - s*[rank m - 1], from the double-double scores.

Finite inputs only (the near-tie contract's NaN / inf rules are the goldens').
"""
from collections import namedtuple

import numpy as np

SPLIT = 134217729.0  # 2^27 + 1 (Veltkamp)


def two_sum(a, b):
    """a + b = s + e exactly (Knuth, no ordering assumed)."""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


def fast_two_sum(a, b):
    """a + b = s + e exactly, given |a| >= |b| (or a == 0)."""
    s = a + b
    e = b - (s - a)
    return s, e


def split(a):
    c = SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """a * b = p + e exactly (Dekker), barring overflow / underflow."""
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dd_add(ah, al, bh, bl):
    """(ah + al) + (bh + bl), relative error <= ~2^-104 (the accurate form)."""
    s, e = two_sum(ah, bh)
    t, f = two_sum(al, bl)
    e = e + t
    s, e = fast_two_sum(s, e)
    e = e + f
    return fast_two_sum(s, e)


def _dd_dots(A, B):
    """(hi, lo) of A B^T for fp64 A (p, d) and B (q, d), column by column."""
    h = np.zeros((A.shape[0], B.shape[0]))
    l = np.zeros_like(h)
    for c in range(A.shape[1]):
        p, e = two_prod(A[:, c][:, None], B[:, c][None, :])
        h, l = dd_add(h, l, p, e)
    return h, l


def dd_gram(X, block=64):
    """(Gh, Gl): the Gram of the rows of X in double-double.  Row blocks keep the
    temporaries in cache and only j >= the block's first row is computed (two_prod
    is exact, so the mirror image is bitwise what the other order gives)."""
    X = np.asarray(X).astype(np.float64)  # fp32 -> fp64 is exact
    n = X.shape[0]
    Gh, Gl = np.empty((n, n)), np.empty((n, n))
    for r in range(0, n, block):
        h, l = _dd_dots(X[r:r + block], X[r:])
        Gh[r:r + block, r:], Gl[r:r + block, r:] = h, l
        Gh[r:, r:r + block], Gl[r:, r:r + block] = h.T, l.T
    return Gh, Gl


def dd_gram_replace_row(G, X, i):
    """The Gram of X from the Gram G = (Gh, Gl) of rows that differ from X's in
    row i alone: row and column i recomputed (bitwise dd_gram(X)), the rest kept.
    A ladder's rungs differ in one row, so each costs O(n d) instead of O(n^2 d)."""
    X = np.asarray(X).astype(np.float64)
    Gh, Gl = G[0].copy(), G[1].copy()
    h, l = _dd_dots(X[i:i + 1], X)
    Gh[i, :], Gl[i, :] = h[0], l[0]
    Gh[:, i], Gl[:, i] = h[0], l[0]
    return Gh, Gl


Exact = namedtuple("Exact", "Gh Gl M D scores scores_lo order sel gap n f k m")


def krum(X, f, gram=None, block=64):
    """The exact Multi-Krum of the rows of X (finite) with f rejected; gram: the
    rows' double-double Gram where the caller already holds it.

    Returns Exact(Gh, Gl, M, D, scores, scores_lo, order, sel, gap, n, f, k, m):
    the double-double Gram, M = max_i G_ii, the fp64 distance matrix (diagonal
    +inf), the scores rounded once and the low words they dropped, the rank order
    of all rows, the ascending selection and the exact boundary gap."""
    X = np.asarray(X)
    assert X.ndim == 2 and np.all(np.isfinite(X))
    n = X.shape[0]
    m, k = n - f, max(0, n - f - 2)
    assert 1 <= f < n
    Gh, Gl = dd_gram(X) if gram is None else gram
    dh, dl = np.diagonal(Gh).copy(), np.diagonal(Gl).copy()
    idx = np.arange(n)
    D, sh, sl = np.empty((n, n)), np.zeros(n), np.zeros(n)
    for r in range(0, n, block):
        rows = idx[r:r + block]
        # G_ii + G_jj - 2 G_ij (the doubling is exact)
        Sh, Sl = dd_add(dh[rows, None], dl[rows, None], dh[None, :], dl[None, :])
        Dh, Dl = dd_add(Sh, Sl, -2.0 * Gh[rows], -2.0 * Gl[rows])
        Dh[rows - r, rows] = np.inf
        Dl[rows - r, rows] = 0.0
        D[rows] = Dh
        # each row ascending by (hi, lo): sort on hi, and order equal hi by lo
        # only in the rows that hold such a pair out of order
        by = np.argsort(Dh, axis=1, kind="stable")
        Rh, Rl = np.take_along_axis(Dh, by, axis=1), np.take_along_axis(Dl, by, axis=1)
        bad = np.nonzero(np.any((Rh[:, 1:] == Rh[:, :-1]) & (Rl[:, 1:] < Rl[:, :-1]), axis=1))[0]
        for i in bad:
            o = np.lexsort((Rl[i], Rh[i]))
            Rh[i], Rl[i] = Rh[i][o], Rl[i][o]
        h, l = np.zeros(len(rows)), np.zeros(len(rows))
        for c in range(k):
            h, l = dd_add(h, l, Rh[:, c], Rl[:, c])
        sh[rows], sl[rows] = h, l
    order = np.lexsort((idx, sl, sh))  # (value, index), the value in double-double
    sel = np.sort(order[:m]).astype(np.int64)
    lo, hi = order[m - 1], order[m]
    gap = float(dd_add(sh[hi], sl[hi], -sh[lo], -sl[lo])[0])
    return Exact(Gh, Gl, float(np.max(dh)), D, sh, sl, order, sel, gap, n, f, k, m)
