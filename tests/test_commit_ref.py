"""The bn256 oracle (tests/commit_ref.py) checked against itself and against
what bk_bn256.h states as numbers: the group order, the fast scalar
multiplication against the literal one, the affine group law, the Horner form of
the witness polynomial against dividePolynomial's, and the Montgomery constants
derived again from p.  No GPU."""
import os
import random
import re

import numpy as np

import commit_ref as C
import shares_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "biscotti_amd", "csrc", "bk_bn256.h")

EDGE = (list(range(-33, 34)) + [(1 << 63) - 1, S.INT64_MIN, 1 << 32, -(1 << 32), (1 << 60) + 1,
                                -((1 << 60) + 1)])


def test_order_and_generator():
    assert C.on_curve(1, C.P - 2)
    assert C.is_inf(C.mul(C.G, C.N))
    # mul reduces first: N G is the empty loop's infinity, so walk the bits
    s = C.INF
    for i in range(C.N.bit_length(), -1, -1):
        s = C.double(s)
        if (C.N >> i) & 1:
            s = C.add(s, C.G)
    assert C.is_inf(s)
    assert C.affine(C.mul(C.G, C.N - 1)) == (1, 2)
    assert C.marshal(C.INF) == C.ZERO64 and C.is_inf(C.unmarshal(C.ZERO64))


def test_fast_equals_literal_on_the_edge_scalars():
    pt = C.mul(C.G, 0x1234567)
    for v in EDGE:
        lit = C.marshal(C.mul(pt, v))
        assert lit == C.marshal(C.mul_fast(pt, v)), v
        if v < 0:
            assert lit == C.marshal(C.mul(pt, C.N + v)), v
    assert C.marshal(C.mul(pt, 0)) == C.ZERO64


def _affine_add(a, b):
    """The chord-and-tangent law on affine points (None: infinity)."""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % C.P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], C.P - 2, C.P) % C.P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], C.P - 2, C.P) % C.P
    x = (lam * lam - a[0] - b[0]) % C.P
    return (x, (lam * (a[0] - x) - a[1]) % C.P)


def test_group_law():
    rng = random.Random(27)
    pts = [C.mul(C.G, rng.randrange(1, C.N)) for _ in range(4)] + [C.INF, C.G]
    for a in pts:
        assert C.affine(C.double(a)) == _affine_add(C.affine(a), C.affine(a))
        assert C.is_inf(C.add(a, C.neg(a)))
        assert C.same(C.add(a, a), C.double(a))
        assert C.same(C.add(a, C.INF), a) and C.same(C.add(C.INF, a), a)
        for b in pts:
            assert C.affine(C.add(a, b)) == _affine_add(C.affine(a), C.affine(b))
            assert C.same(C.add(a, b), C.add(b, a))
    a, b, c = pts[:3]
    assert C.same(C.add(C.add(a, b), c), C.add(a, C.add(b, c)))
    k, m = rng.randrange(C.N), rng.randrange(C.N)
    assert C.same(C.add(C.mul(C.G, k), C.mul(C.G, m)), C.mul(C.G, k + m))
    for a in pts:
        assert C.same(C.unmarshal(C.marshal(a)), a)
    bad = bytearray(C.marshal(C.G))
    bad[63] ^= 1
    assert C.unmarshal(bad) is None
    assert C.unmarshal(C.P.to_bytes(32, "big") + (2).to_bytes(32, "big")) is None


def _large(d):
    """tests/test_gpu_shares.py's _large."""
    rng = np.random.default_rng(5000 + d)
    v = rng.uniform(-1e11, 1e11, size=d)
    for i, x in zip(range(0, d, 7), [np.nan, np.inf, -np.inf, 1e300, -0.0] * d):
        v[i] = x
    return v


def test_horner_quotient_equals_divide_polynomial():
    cases = []
    for d in (25, 70):
        q = S.quantize(_large(d), 4)
        assert S.INT64_MIN in q
        cases += S.chunks_of(q, 10)
    rng = random.Random(5)
    cases += [[rng.randrange(-10 ** 6, 10 ** 6) for _ in range(L)] for L in (1, 2, 3, 9, 10)]
    # leading coefficients 0: dividePolynomial's quotient is shorter
    cases += [[5, -7, 3, 0, 0], [0, 0, 0], [4, 0], [0, 9, 0, 0, 0, 0, 0, 0, 0, 0],
              [S.INT64_MIN] * 10, [(1 << 63) - 1] * 10]
    for coefs in cases:
        for s in range(21):
            lit = C.witness_polynomial(coefs, s)
            assert lit[-1] == 0
            hor = C.witness_horner(coefs, s)
            assert len(hor) == len(coefs) - 1
            # the literal form drops what lies above the degree: zeros in Horner's
            assert lit[:-1] + [0] * (len(hor) - len(lit) + 1) == hor, (coefs, s)
    assert C.witness_polynomial([7], 3) == [0]


def _limbs(name):
    text = open(HEADER).read()
    m = re.search(r"constexpr uint32_t " + name + r"\[8\] = \{([^}]*)\}", text)
    assert m, name
    w = [int(t.strip().rstrip("u"), 16) for t in m.group(1).split(",")]
    assert len(w) == 8
    return sum(v << (32 * i) for i, v in enumerate(w))


def test_montgomery_constants():
    R = 1 << 256
    assert _limbs("FP_P") == C.P
    assert _limbs("FP_PM2") == C.P - 2
    assert _limbs("FP_R1") == R % C.P
    assert _limbs("FP_R2") == R * R % C.P
    assert _limbs("FP_B3") == 3 * R % C.P
    m = re.search(r"FP_NP = (0x[0-9a-f]+)u", open(HEADER).read())
    assert int(m.group(1), 16) == (-pow(C.P, -1, 1 << 32)) % (1 << 32)
    assert C.P.bit_length() == 256 and C.N.bit_length() == 256
    m = re.search(r"WINDOW_BIAS = (0x[0-9a-f]+)ull", open(HEADER).read())
    assert int(m.group(1), 16) == sum(8 << (4 * w) for w in range(16))
