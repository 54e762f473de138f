"""The secure-aggregation share arithmetic in pure Python integers and floats,
written from DistSys/kyber.go (test infrastructure only).

    quantize              updateFloatToInt, kyber.go:698-710
    share_value_literal   createShareAndWitness's evaluatedValue, kyber.go:579-646,
                          with dividePolynomial (kyber.go:768-793) as written
    share_value_horner    the same value with the division as a Horner recurrence
    recover_exact         the integer polynomial through the first P points
                          (Newton divided differences, exact divisions), checked
                          modulo 2^64 against all points
    recover_float         recoverSecret's method (kyber.go:809-857): fp64 least
                          squares on the Vandermonde matrix, then rounding --
                          numpy's lstsq standing in for gonum's QR

A Python float is an IEEE double and every operation on it rounds on its own,
as Go's amd64 code does.  One assumption cannot be checked without Go: that
math.Pow(x, j) returns the exact integer power for the |x| <= 53, j <= 9 used
here (those powers are below 2^53, so exact doubles exist); the powers here are
built by integer multiplication.
"""
import numpy as np

INT64_MIN = -(1 << 63)
X0 = 10  # share s sits at x = s - 10 (pointToHashVal, kyber.go:677-695)


def wrap(v):
    """An integer as a wrapping int64."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def go_int64(f):
    """Go's int64(float64) on amd64: truncation; NaN and out-of-range values
    give the 'integer indefinite' INT64_MIN."""
    if f != f or f >= 9223372036854775808.0 or f < -9223372036854775808.0:
        return INT64_MIN
    return int(f)


def quantize(delta, precision):
    scale = 1.0
    for _ in range(precision):
        scale *= 10.0
    return [go_int64(float(v) * scale) for v in delta]


def chunks_of(q, poly_size):
    return [q[i:i + poly_size] for i in range(0, len(q), poly_size)]


def _degree(p):
    for d in range(len(p) - 1, -1, -1):
        if p[d] != 0:
            return d
    return -1


def divide_polynomial(nn, dd):
    """kyber.go:768-793, line by line."""
    if _degree(dd) < 0:
        return None, None
    q = []
    nnfloat = list(nn)
    if _degree(nnfloat) >= _degree(dd):
        q = [0.0] * (_degree(nnfloat) - _degree(dd) + 1)
        while _degree(nnfloat) >= _degree(dd):
            d = [0.0] * (_degree(nnfloat) + 1)
            k = _degree(nnfloat) - _degree(dd)
            for i, v in enumerate(dd[:len(d) - k]):
                d[k + i] = v
            q[_degree(nnfloat) - _degree(dd)] = nnfloat[_degree(nnfloat)] / d[_degree(d)]
            for i in range(len(d)):
                d[i] *= q[_degree(nnfloat) - _degree(dd)]
                nnfloat[i] -= d[i]
    return q, nnfloat


def share_value_literal(update, s):
    """createShareAndWitness's evaluatedValue for the int64 coefficients
    `update` and share index s."""
    uf = [float(c) for c in update]
    x = s - X0
    y = 0
    for i in range(len(uf)):
        y = wrap(y + go_int64(float(x ** i) * uf[i]))
    uf[0] = float(wrap(go_int64(uf[0]) - y))
    _, rem = divide_polynomial(uf, [float(x * -1), 1.0])
    return wrap(y + go_int64(rem[0] * 1.0))


def share_value_horner(update, s):
    cf = [float(c) for c in update]
    x = s - X0
    xd, nx = float(x), float(-x)
    y, pw = 0, 1.0
    for j in range(len(cf)):
        y = wrap(y + go_int64(pw * cf[j]))
        pw = pw * xd
    c0 = float(wrap(go_int64(cf[0]) - y))
    h = 0.0
    for k in range(len(cf) - 1, 0, -1):
        h = cf[k] - nx * h
    h = c0 - nx * h
    return wrap(y + go_int64(h * 1.0))


def generate(delta, precision, poly_size, total_shares, value=share_value_horner):
    """[chunk][share] int64, the layout of bk_shares_generate's y_out."""
    ch = chunks_of(quantize(delta, precision), poly_size)
    out = np.empty((len(ch), total_shares), dtype=np.int64)
    for c, coefs in enumerate(ch):
        for s in range(total_shares):
            out[c, s] = value(coefs, s)
    return out


def recover_exact(xs, ys, poly_size):
    """The integer coefficients (poly_size of them) of the polynomial through
    the first poly_size points, or None for a bad chunk: an inexact division, a
    coefficient outside int64, or a point (of all of them) not reproduced
    modulo 2^64."""
    P = poly_size
    xs = [int(x) for x in xs]
    ys = [int(y) for y in ys]
    dd = ys[:P]
    for k in range(1, P):
        for i in range(P - 1, k - 1, -1):
            num, den = dd[i] - dd[i - 1], xs[i] - xs[i - k]
            if num % den:
                return None
            dd[i] = num // den
    m = [0] * P
    for k in range(P - 1, -1, -1):
        for j in range(P - 1, 0, -1):
            m[j] = m[j - 1] - xs[k] * m[j]
        m[0] = dd[k] - xs[k] * m[0]
    if any(not INT64_MIN <= c < (1 << 63) for c in m):
        return None
    for x, y in zip(xs, ys):
        v = 0
        for c in reversed(m):
            v = v * x + c
        if wrap(v) != y:
            return None
    return m


def recover_float(xs, ys, poly_size):
    """(rounded int64 coefficients, the float solution) by recoverSecret's
    method."""
    A = np.vander(np.asarray(xs, dtype=np.float64), poly_size, increasing=True)
    sol = np.linalg.lstsq(A, np.asarray(ys, dtype=np.float64), rcond=None)[0]
    return np.rint(sol).astype(np.int64), sol


def wrapping_sum(arrays):
    """Element-wise wrapping int64 sum (numpy's integer add wraps)."""
    acc = np.zeros_like(np.asarray(arrays[0], dtype=np.int64))
    for a in arrays:
        acc = acc + np.asarray(a, dtype=np.int64)
    return acc
