"""The bn256 G1 commitments in pure Python integers, written from
DistSys/kyber.go and kyber's pairing/bn256 (test infrastructure only).

    add, double, mul        curvePoint.Add / Double / Mul: Jacobian coordinates,
                            add-2007-bl and dbl-2009-l, double-and-add from
                            BitLen() down on the scalar reduced modulo the order
    marshal, unmarshal      pointG1.MarshalBinary / UnmarshalBinary
    create_commitment       createCommitment, kyber.go:533-562 (SetInt64 = v mod n)
    witness_polynomial      createShareAndWitness's qInt, kyber.go:579-646, with
                            shares_ref.divide_polynomial and go_int64 as they are
    witness_horner          the same coefficients as Horner intermediates
    mul_fast, commit_fast   v P = |v| (-P), for the larger cases
    generate                the three outputs of generateMinerSecretShares'
                            commitments (kyber.go:456-482, 172-202)

A point is a tuple (x, y, z) of integers modulo p; z = 0 is infinity.  Field
elements are plain residues: Montgomery form changes no result.
"""
import numpy as np

import shares_ref as S

P = 65000549695646603732796438742359905742825358107623003571877145026864184071783
N = 65000549695646603732796438742359905742570406053903786389881062969044166799969
B = 3
G = (1, P - 2, 1)
INF = (0, 1, 0)
ZERO64 = bytes(64)


def is_inf(a):
    return a[2] % P == 0


def double(a):
    x, y, z = a
    A = x * x % P
    Bq = y * y % P
    C = Bq * Bq % P
    t = (x + Bq) % P
    t2 = t * t % P
    t = (t2 - A) % P
    t2 = (t - C) % P
    d = (t2 + t2) % P
    t = (A + A) % P
    e = (t + A) % P
    f = e * e % P
    t = (d + d) % P
    cx = (f - t) % P
    t = (C + C) % P
    t2 = (t + t) % P
    t = (t2 + t2) % P
    cy = (d - cx) % P
    t2 = e * cy % P
    cy = (t2 - t) % P
    t = y * z % P
    cz = (t + t) % P
    return (cx, cy, cz)


def add(a, b):
    if is_inf(a):
        return b
    if is_inf(b):
        return a
    z12 = a[2] * a[2] % P
    z22 = b[2] * b[2] % P
    u1 = a[0] * z22 % P
    u2 = b[0] * z12 % P
    t = b[2] * z22 % P
    s1 = a[1] * t % P
    t = a[2] * z12 % P
    s2 = b[1] * t % P
    h = (u2 - u1) % P
    x_equal = h == 0
    t = (h + h) % P
    i = t * t % P
    j = h * i % P
    t = (s2 - s1) % P
    y_equal = t == 0
    if x_equal and y_equal:
        return double(a)
    r = (t + t) % P
    v = u1 * i % P
    t4 = r * r % P
    t = (v + v) % P
    t6 = (t4 - j) % P
    cx = (t6 - t) % P
    t = (v - cx) % P
    t4 = s1 * j % P
    t6 = (t4 + t4) % P
    t4 = r * t % P
    cy = (t4 - t6) % P
    t = (a[2] + b[2]) % P
    t4 = t * t % P
    t = (t4 - z12) % P
    t4 = (t - z22) % P
    cz = t4 * h % P
    return (cx, cy, cz)


def neg(a):
    return (a[0], (-a[1]) % P, a[2])


def mul(a, scalar):
    """curvePoint.Mul on mod.Int's value: the scalar modulo the order."""
    scalar %= N
    s = INF
    for i in range(scalar.bit_length(), -1, -1):
        t = double(s)
        s = add(t, a) if (scalar >> i) & 1 else t
    return s


def mul_fast(a, v):
    """v a for a signed v through |v| (-a): the same point as mul(a, v)."""
    if v < 0:
        a, v = neg(a), -v
    s = INF
    for i in range(v.bit_length(), -1, -1):
        s = double(s)
        if (v >> i) & 1:
            s = add(s, a)
    return s


def affine(a):
    if is_inf(a):
        return None
    zi = pow(a[2], P - 2, P)
    zi2 = zi * zi % P
    return (a[0] * zi2 % P, a[1] * zi % P * zi2 % P)


def marshal(a):
    xy = affine(a)
    if xy is None:
        return ZERO64
    return xy[0].to_bytes(32, "big") + xy[1].to_bytes(32, "big")


def on_curve(x, y):
    return (y * y - x * x * x - B) % P == 0


def unmarshal(buf):
    """The point, or None where UnmarshalBinary fails (this package also
    refuses a coordinate >= p, which kyber's montEncode would reduce)."""
    buf = bytes(buf)
    assert len(buf) == 64
    x, y = int.from_bytes(buf[:32], "big"), int.from_bytes(buf[32:], "big")
    if x >= P or y >= P:
        return None
    if x == 0 and y == 0:
        return INF
    if not on_curve(x, y):
        return None
    return (x, y, 1)


def same(a, b):
    return marshal(a) == marshal(b)


def create_commitment(update, key, times=mul):
    c = INF
    for i in range(len(update)):
        c = add(c, times(key[i], int(update[i])))
    return c


def commit_fast(update, key):
    return create_commitment(update, key, mul_fast)


def witness_polynomial(update, s):
    """createShareAndWitness's qInt (with its appended 0) for the int64
    coefficients `update` and share index s."""
    uf = [float(c) for c in update]
    x = s - S.X0
    y = 0
    for i in range(len(uf)):
        y = S.wrap(y + S.go_int64(float(x ** i) * uf[i]))
    uf[0] = float(S.wrap(S.go_int64(uf[0]) - y))
    quotient, _ = S.divide_polynomial(uf, [float(x * -1), 1.0])
    return [S.go_int64(q * 1.0) for q in quotient] + [0]


def witness_horner(update, s):
    """len(update) - 1 coefficients: h <- c_k - (-x) h for k = L-1 .. 1."""
    cf = [float(c) for c in update]
    nx = float(-(s - S.X0))
    q = [0] * (len(cf) - 1)
    h = 0.0
    for k in range(len(cf) - 1, 0, -1):
        h = cf[k] - nx * h
        q[k - 1] = S.go_int64(h)
    return q


def generate(q, key, poly_size, total_shares, times=mul_fast, witness=witness_polynomial,
             chunks=None):
    """(commitment, chunk commitments, witnesses) of the quantised update q as
    64-byte strings: bytes, [chunk] and [chunk][share].  chunks: the chunk
    numbers whose witnesses are wanted (None: all)."""
    q = [int(v) for v in q]
    whole = marshal(create_commitment(q, key, times))
    ch = S.chunks_of(q, poly_size)
    cc, ww = [], {}
    for c, coefs in enumerate(ch):
        sub = key[c * poly_size:c * poly_size + len(coefs)]
        cc.append(marshal(create_commitment(coefs, sub, times)))
        if chunks is not None and c not in chunks:
            continue
        row = []
        for s in range(total_shares):
            qi = witness(coefs, s)
            # qInt may be longer than the key slice only by its trailing 0
            row.append(marshal(create_commitment(qi[:len(sub)], sub, times)))
        ww[c] = row
    return whole, cc, ww


def key_powers(count):
    """GenerateKey's PKG1 with secret 2: PK[i] = 2^i G."""
    key, a = [], G
    for _ in range(count):
        key.append(a)
        a = double(a)
    return key


def key_bytes(key):
    return b"".join(marshal(a) for a in key)


def as_array(blobs):
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(len(blobs), 64).copy()
