"""Inputs and the flag-contract check shared by tests/test_exact_ref.py (CPU, the
oracle as the implementation) and tests/test_gpu_exact_scores.py (every GPU
path): seeded numpy, checked against tests/exact_ref.py.

cluster(n, d, f, ratio)    honest rows mu + z / ratio, f Byzantine rows with
                           + 3 z' on top.  The honest scores are ~ratio^2 below
                           the Gram's magnitude M (which the Byzantine rows
                           carry): the cancellation regime of a federated round,
                           where G_ii + G_jj - 2 G_ij loses 2 log2(ratio) bits.
ladder(n, d, f, ratio, t)  cluster with f - 1 Byzantine rows, and two more rows
                           a = mu + 4 w / ratio and b = a + 2^-t v / ratio that
                           score above every honest row and below every
                           Byzantine one: {a, b} sit at ranks m - 1 and m, and the
                           boundary gap shrinks ~2x per step of t.  t = None:
                           b = a, an exact tie.
"""
import numpy as np

import exact_ref as XR
import golden_util as GU


QUIET = 2.0 ** -20


def _base(n, d, nbyz, ratio, seed, skip=(), quiet=0):
    rng = np.random.default_rng(seed)
    scale = np.ones(d)
    scale[d - quiet:] = QUIET
    mu = rng.standard_normal(d) * scale
    X = mu + rng.standard_normal((n, d)) * scale / ratio
    free = np.setdiff1d(np.arange(n), np.asarray(skip, dtype=np.int64))
    byz = np.sort(rng.choice(free, nbyz, replace=False))
    X[byz] += 3.0 * rng.standard_normal((nbyz, d)) * scale
    return rng, mu, X, scale


def cluster(n, d, f, ratio, seed=1, dtype=np.float64, quiet=0):
    _, _, X, _ = _base(n, d, f, ratio, seed, quiet=quiet)
    return np.ascontiguousarray(X.astype(dtype))


def ladder_pair(n):
    """The rows a and b of ladder(): fixed by n alone, a below b."""
    return n // 3, (2 * n) // 3 + 1


def ladder(n, d, f, ratio, t, seed=1, dtype=np.float64, quiet=0):
    ia, ib = ladder_pair(n)
    rng, mu, X, scale = _base(n, d, f - 1, ratio, seed, skip=(ia, ib), quiet=quiet)
    w, v = rng.standard_normal(d), rng.standard_normal(d)
    X[ia] = mu + 4.0 * w * scale / ratio
    X[ib] = X[ia] if t is None else X[ia] + 2.0 ** -t * v / ratio
    return np.ascontiguousarray(X.astype(dtype))


def check_rung(ex, sel, scores, near_tie, err_bound, e_here, pair=None, tie=False):
    """The score and flag contract of one call against the exact reference ex:
    every score within e_here; near_tie = 0 proves the exact selection; a gap
    that clears err_bound + 2 e_here is not flagged; an exact tie is flagged and
    goes to the lower index.  Returns max |s - s*|."""
    err = float(np.max(np.abs(scores - ex.scores)))
    assert err <= e_here, "score error %.3e > e_here %.3e" % (err, e_here)
    if not near_tie:
        assert np.array_equal(sel, ex.sel), "near_tie = 0 but not the exact selection"
    if ex.gap > err_bound + 2.0 * e_here:
        assert not near_tie, "gap %.3e clears %.3e yet flagged" % (ex.gap, err_bound + 2 * e_here)
    if pair is not None:  # the ladder's design: {a, b} at ranks m - 1, m
        assert {int(ex.order[ex.m - 1]), int(ex.order[ex.m])} == set(pair)
    if tie:
        assert ex.gap == 0.0 and near_tie
        assert min(pair) in sel and max(pair) not in sel
    return err


def flag_of(scores, M, d, f, u_gram=2.0 ** -53, eg=0.0):
    """bk_selection_margin's record from a score vector, as write_margin does:
    (sel, gap, err_bound, near_tie, e_here)."""
    n = len(scores)
    m, k = n - f, max(0, n - f - 2)
    order = np.lexsort((np.arange(n), scores))
    gap = float(scores[order[m]] - scores[order[m - 1]])
    e_here, _ = GU.margin_e(M, d, k, u_gram, eg)
    bound = GU.margin_bound(M, d, k, u_gram, eg)
    return np.sort(order[:m]), gap, bound, not gap > bound, e_here


# ---- the cases of tests/test_gpu_exact_scores.py ------------------------------
# Rungs (values of t, then the tie None) were chosen on the CPU from the bound
# formula and the exact gaps, at least 4x away from err_bound on either side
# wherever the shape allows: the first entries clear the bound, the last ones sit
# under it.  fp32 rows cannot hold a difference below ulp(a_c), and the fp64 bound
# is ~2^-35 of M, so the fp32 ladders of the exact paths keep 8 quiet trailing
# columns (every row 2^-20 of the others there): from t ~ 28 on b - a lives in
# them alone, a nonzero gap far under the bound.  The approximate modes' bounds
# are ~2^29 larger (fp32 MFMA, two int8 digits), so their ladders start at
# negative t and their rows need no quiet columns.
F64_RUNGS = (0, 4, 8, 16, 24, 32, None)
F32_RUNGS = (8, 16, 24, 28, 32, 36, None)
BIG_RUNGS = (0, 4, 16, 24, None)


def _case(cid, n, d, f, dtype, ratio, rungs, ld=None, quiet=0, entry="device", mode=None,
          cert=None, u_gram=2.0 ** -53, int8=False):
    return dict(id=cid, n=n, d=d, ld=ld or d, f=f, dtype=dtype, ratio=ratio, rungs=rungs,
                quiet=quiet, entry=entry, mode=mode, cert=cert, u_gram=u_gram, int8=int8)


def _exact_pair(name, n, d, f, ratio64):
    return [_case("%s-f64-%dx%d" % (name, n, d), n, d, f, np.float64, ratio64, F64_RUNGS),
            _case("%s-f32-%dx%d" % (name, n, d), n, d, f, np.float32, 2.0 ** 4, F32_RUNGS, quiet=8)]


CASES = [
    # the general chain, n = 130: K1 v3 / v1, fp64 and fp32 rows widened
    _case("chain-f64-ld70-K1v3", 130, 70, 40, np.float64, 2.0 ** 10, F64_RUNGS),
    _case("chain-f64-ld71-K1v1", 130, 70, 40, np.float64, 2.0 ** 10, F64_RUNGS, ld=71),
    _case("chain-f32-ld72-K1v3", 130, 72, 40, np.float32, 2.0 ** 4, F32_RUNGS, quiet=8),
    _case("chain-f32-ld70-K1v1", 130, 70, 40, np.float32, 2.0 ** 4, F32_RUNGS, quiet=8),
    # 257 k-blocks over K1's 256 workgroups: every tile is a sum of split-K partials (K1b)
    _case("chain-f64-d4100-splitK-K1b", 130, 4100, 40, np.float64, 2.0 ** 10, F64_RUNGS),
    # large n: more than one workgroup group; the lane-exchange and the transposed K2
    _case("chain-f64-1100x70-K2lane", 1100, 70, 330, np.float64, 2.0 ** 10, BIG_RUNGS),
    _case("chain-f64-2100x8-K2transposed", 2100, 8, 630, np.float64, 2.0 ** 10, BIG_RUNGS),
] + _exact_pair("k_tiny", 16, 25, 5, 2.0 ** 10) + _exact_pair("k_small", 17, 25, 5, 2.0 ** 10) \
  + _exact_pair("k_small", 100, 785, 30, 2.0 ** 6) + _exact_pair("k_small", 128, 70, 40, 2.0 ** 10) + [
    # the incremental collection: k_border's Gram, the one-launch and the chain finish
    _case("collect-f64-100x785-onelaunch", 100, 785, 30, np.float64, 2.0 ** 6, F64_RUNGS,
          entry="collect"),
    _case("collect-f64-130x70-chain", 130, 70, 40, np.float64, 2.0 ** 10, F64_RUNGS,
          entry="collect"),
    # the approximate Grams at 130 x 72, each with its certified sibling
    _case("mode-f32-MFMA", 130, 72, 40, np.float32, 2.0 ** 4, (-4, -2, 0, 6, 8, 12, None),
          mode="BK_F32_MFMA", cert="BK_F32_CERTIFIED", u_gram=2.0 ** -24),
    _case("mode-f32-I8", 130, 72, 40, np.float32, 2.0 ** 4, (-5, -4, -2, 2, 4, 8, None),
          mode="BK_F32_I8", cert="BK_F32_I8_CERTIFIED", int8=True),
    _case("mode-f32-I8X2", 130, 72, 40, np.float32, 2.0 ** 4, (-5, -4, -2, 0, 4, None),
          mode="BK_F32_I8X2", cert="BK_F32_I8X2_CERTIFIED", int8=True),
    _case("mode-f64-I8", 130, 72, 40, np.float64, 2.0 ** 4, (-5, -4, -2, 2, 4, 8, None),
          mode="BK_F64_I8", cert="BK_F64_I8_CERTIFIED", int8=True),
    _case("mode-f64-I8X2", 130, 72, 40, np.float64, 2.0 ** 4, (-5, -4, -2, 0, 4, None),
          mode="BK_F64_I8X2", cert="BK_F64_I8X2_CERTIFIED", int8=True),
]
CASE_IDS = [c["id"] for c in CASES]


_RUNGS = {}


def rung_inputs(case):
    """[(t, X, exact)] of a case's ladder: one double-double Gram for the tie's
    rows, row b's row and column replaced per rung.  Computed once per distinct
    input and shared (read-only) by every test that asks."""
    n, d, f = case["n"], case["d"], case["f"]
    key = (n, d, f, case["dtype"], case["ratio"], case["quiet"], case["rungs"])
    if key in _RUNGS:
        return _RUNGS[key]
    kw = dict(dtype=case["dtype"], quiet=case["quiet"])
    ib = ladder_pair(n)[1]
    X0 = ladder(n, d, f, case["ratio"], None, **kw)
    G0 = XR.dd_gram(X0)
    out = []
    for t in case["rungs"]:
        X = ladder(n, d, f, case["ratio"], t, **kw)
        G = G0 if t is None else XR.dd_gram_replace_row(G0, X, ib)
        ex = XR.krum(X, f, gram=G, block=64 if n <= 256 else 256)
        if n > 256:  # the (n, n) arrays of the large cases are not kept
            ex = ex._replace(Gh=None, Gl=None, D=None)
        X.setflags(write=False)
        out.append((t, X, ex))
    _RUNGS[key] = out
    return out


def exact_path(case):
    """u_G = 2^-53 and no int8 term: the paths the sharper, measured gate covers."""
    return case["u_gram"] == 2.0 ** -53 and not case["int8"]
