// bk_bn256.h -- the G1 arithmetic of bn256 behind bk_commit_* (DESIGN.md §5w),
// for host and device code alike: GF(p) in Montgomery form (R = 2^256), the
// curve y^2 = x^3 + 3 in Jacobian coordinates, 64-bit signed scalars and the
// 64-byte marshalling of pointG1.MarshalBinary (affine x, then y, big-endian).
//
// p fills all 256 bits, so a sum of two residues can carry out of the top limb:
// fp_add and fp_mul carry that bit into their final subtraction.  A field
// element is 8 x 32-bit limbs, least significant first; every loop over limbs is
// fully unrolled and indexed by its counter only, so device code keeps the limbs
// in registers (the rule of bk_shares.hip).  The constants below are numbers;
// tests/test_commit_ref.py derives each of them again from p.
//
// Every result is canonical: a marshalled point is the same 64 bytes whatever
// the order of the additions that led to it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BK_HD __host__ __device__ __forceinline__
#else
#define BK_HD inline
#endif
#if defined(__clang__)
#define BK_UNROLL _Pragma("unroll")
#else
#define BK_UNROLL
#endif

namespace bk {
namespace bn {

// p = 65000549695646603732796438742359905742825358107623003571877145026864184071783
constexpr uint32_t FP_P[8] = {0x5e089667u, 0x185cac6cu, 0x20b5b59eu, 0xee5b88d1u,
                              0x6184dc21u, 0xaa6fecb8u, 0x4aa387f9u, 0x8fb501e3u};
// p - 2 (Fermat's exponent)
constexpr uint32_t FP_PM2[8] = {0x5e089665u, 0x185cac6cu, 0x20b5b59eu, 0xee5b88d1u,
                                0x6184dc21u, 0xaa6fecb8u, 0x4aa387f9u, 0x8fb501e3u};
// R mod p (one), R^2 mod p, 3 R mod p (the curve's b)
constexpr uint32_t FP_R1[8] = {0xa1f76999u, 0xe7a35393u, 0xdf4a4a61u, 0x11a4772eu,
                               0x9e7b23deu, 0x55901347u, 0xb55c7806u, 0x704afe1cu};
constexpr uint32_t FP_R2[8] = {0x7e444f56u, 0x9c21c3ffu, 0xb2efb0c2u, 0x409ed151u,
                               0x80fb1651u, 0x0c6dc37bu, 0x2c2380b7u, 0x7c36e0e6u};
constexpr uint32_t FP_B3[8] = {0x29d50ffdu, 0x8630a1e2u, 0x5c7373e9u, 0x583653eau,
                               0x1867b356u, 0xabd06066u, 0x8ace581fu, 0x3176f68fu};
// -p^-1 mod 2^32
constexpr uint32_t FP_NP = 0x7f17daa9u;

struct Fp {
    uint32_t v[8];
};

BK_HD Fp fp_const(const uint32_t (&k)[8]) {
    Fp r;
BK_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = k[i];
    return r;
}
BK_HD Fp fp_zero() {
    Fp r;
BK_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = 0u;
    return r;
}
BK_HD Fp fp_one() { return fp_const(FP_R1); }

BK_HD bool fp_is_zero(const Fp &a) {
    uint32_t o = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) o |= a.v[i];
    return o == 0u;
}
BK_HD bool fp_eq(const Fp &a, const Fp &b) {
    uint32_t o = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) o |= a.v[i] ^ b.v[i];
    return o == 0u;
}

// a >= p, for any 256-bit a
BK_HD bool fp_geq_p(const Fp &a) {
    uint64_t br = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) br = ((uint64_t)a.v[i] - FP_P[i] - br) >> 63;
    return br == 0;
}

// (hi 2^256 + a) - p where that is not negative, else a: the value below p of
// any hi 2^256 + a < 2 p
BK_HD Fp fp_reduce_once(const Fp &a, uint32_t hi) {
    Fp s;
    uint64_t br = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)a.v[i] - FP_P[i] - br;
        s.v[i] = (uint32_t)t;
        br = t >> 63;
    }
    const bool take = hi != 0u || br == 0;
    Fp r;
BK_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = take ? s.v[i] : a.v[i];
    return r;
}

BK_HD Fp fp_add(const Fp &a, const Fp &b) {
    Fp s;
    uint64_t c = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.v[i] + b.v[i];
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return fp_reduce_once(s, (uint32_t)c);
}

BK_HD Fp fp_sub(const Fp &a, const Fp &b) {
    Fp s;
    uint64_t br = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)a.v[i] - b.v[i] - br;
        s.v[i] = (uint32_t)t;
        br = t >> 63;
    }
    // a borrow: add p back (the carry out of the top limb cancels the borrow)
    const uint32_t m = br ? 0xffffffffu : 0u;
    uint64_t c = 0;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)s.v[i] + (FP_P[i] & m);
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return s;
}

BK_HD Fp fp_neg(const Fp &a) { return fp_sub(fp_zero(), a); }
BK_HD Fp fp_dbl(const Fp &a) { return fp_add(a, a); }

// a b / R mod p: the coarsely integrated operand scan, one 32x32+64
// multiply-add per limb pair
BK_HD Fp fp_mul(const Fp &a, const Fp &b) {
    uint32_t t[10];
BK_UNROLL
    for (int i = 0; i < 10; ++i) t[i] = 0u;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
BK_UNROLL
        for (int j = 0; j < 8; ++j) {
            c += (uint64_t)a.v[j] * b.v[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[8] = (uint32_t)c;
        t[9] = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * FP_NP;
        c = (uint64_t)m * FP_P[0] + t[0];
        c >>= 32;
BK_UNROLL
        for (int j = 1; j < 8; ++j) {
            c += (uint64_t)m * FP_P[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (uint32_t)c;
        t[8] = t[9] + (uint32_t)(c >> 32);
    }
    Fp r;
BK_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = t[i];
    return fp_reduce_once(r, t[8]);
}

BK_HD Fp fp_sqr(const Fp &a) { return fp_mul(a, a); }
BK_HD Fp fp_to_mont(const Fp &a) { return fp_mul(a, fp_const(FP_R2)); }
BK_HD Fp fp_from_mont(const Fp &a) {
    Fp one = fp_zero();
    one.v[0] = 1u;
    return fp_mul(a, one);
}

// a^(p-2), Fermat's inverse (0 for a = 0).  The loop is a real loop: two
// multiplications' worth of code
BK_HD Fp fp_inv(const Fp &a) {
    Fp r = fp_one();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 255; bit >= 0; --bit) {
        r = fp_sqr(r);
        uint32_t w = 0;
BK_UNROLL
        for (int i = 0; i < 8; ++i) w = (bit >> 5) == i ? FP_PM2[i] : w;
        if ((w >> (bit & 31)) & 1u) r = fp_mul(r, a);
    }
    return r;
}

// 32 big-endian bytes <-> limbs (not Montgomery form)
BK_HD Fp fp_from_bytes(const uint8_t *b) {
    Fp r;
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint8_t *q = b + 28 - 4 * i;
        r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    return r;
}
BK_HD void fp_to_bytes(const Fp &a, uint8_t *b) {
BK_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint8_t *q = b + 28 - 4 * i;
        q[0] = (uint8_t)(a.v[i] >> 24);
        q[1] = (uint8_t)(a.v[i] >> 16);
        q[2] = (uint8_t)(a.v[i] >> 8);
        q[3] = (uint8_t)a.v[i];
    }
}

// ---- the curve ------------------------------------------------------------

// An affine point in Montgomery form; infinity is (0, 0), which is not on the
// curve (0 != 3)
struct Aff {
    Fp x, y;
};
// Jacobian (X / Z^2, Y / Z^3); infinity is Z = 0 with X, Y arbitrary
struct Jac {
    Fp x, y, z;
};

BK_HD Aff aff_inf() { return Aff{fp_zero(), fp_zero()}; }
BK_HD bool aff_is_inf(const Aff &a) { return fp_is_zero(a.x) && fp_is_zero(a.y); }
BK_HD Aff aff_neg(const Aff &a) { return Aff{a.x, fp_neg(a.y)}; }  // -(0, 0) = (0, 0)
BK_HD Jac jac_inf() { return Jac{fp_one(), fp_one(), fp_zero()}; }
BK_HD bool jac_is_inf(const Jac &a) { return fp_is_zero(a.z); }
BK_HD Jac jac_from_aff(const Aff &a) {
    return aff_is_inf(a) ? jac_inf() : Jac{a.x, a.y, fp_one()};
}

BK_HD bool aff_on_curve(const Aff &a) {
    const Fp y2 = fp_sqr(a.y);
    const Fp x3 = fp_add(fp_mul(fp_sqr(a.x), a.x), fp_const(FP_B3));
    return fp_eq(y2, x3);
}

// 2 a (dbl-2009-l, a = 0).  Infinity stays infinity (Z3 = 2 Y 0); the curve has
// no point of order 2
BK_HD Jac jac_dbl(const Jac &a) {
    const Fp A = fp_sqr(a.x), B = fp_sqr(a.y), C = fp_sqr(B);
    Fp t = fp_sqr(fp_add(a.x, B));
    t = fp_sub(fp_sub(t, A), C);
    const Fp D = fp_dbl(t);
    const Fp E = fp_add(fp_dbl(A), A);
    const Fp F = fp_sqr(E);
    Jac r;
    r.x = fp_sub(F, fp_dbl(D));
    const Fp C8 = fp_dbl(fp_dbl(fp_dbl(C)));
    r.y = fp_sub(fp_mul(E, fp_sub(D, r.x)), C8);
    r.z = fp_dbl(fp_mul(a.y, a.z));
    return r;
}

// a + b for an affine b (madd-2007-bl), complete: either may be infinity, equal
// operands double, opposite operands give infinity
BK_HD Jac jac_add_aff(const Jac &a, const Aff &b) {
    if (aff_is_inf(b)) return a;
    if (jac_is_inf(a)) return Jac{b.x, b.y, fp_one()};
    const Fp z1z1 = fp_sqr(a.z);
    const Fp u2 = fp_mul(b.x, z1z1);
    const Fp s2 = fp_mul(fp_mul(b.y, a.z), z1z1);
    const Fp h = fp_sub(u2, a.x);
    const Fp rr = fp_sub(s2, a.y);
    if (fp_is_zero(h)) {
        if (fp_is_zero(rr)) return jac_dbl(a);
        return jac_inf();
    }
    const Fp hh = fp_sqr(h);
    const Fp i = fp_dbl(fp_dbl(hh));
    const Fp j = fp_mul(h, i);
    const Fp r = fp_dbl(rr);
    const Fp v = fp_mul(a.x, i);
    Jac o;
    o.x = fp_sub(fp_sub(fp_sqr(r), j), fp_dbl(v));
    o.y = fp_sub(fp_mul(r, fp_sub(v, o.x)), fp_dbl(fp_mul(a.y, j)));
    o.z = fp_sub(fp_sub(fp_sqr(fp_add(a.z, h)), z1z1), hh);
    return o;
}

// a + b (add-2007-bl), complete in the same sense
BK_HD Jac jac_add(const Jac &a, const Jac &b) {
    if (jac_is_inf(b)) return a;
    if (jac_is_inf(a)) return b;
    const Fp z1z1 = fp_sqr(a.z), z2z2 = fp_sqr(b.z);
    const Fp u1 = fp_mul(a.x, z2z2), u2 = fp_mul(b.x, z1z1);
    const Fp s1 = fp_mul(fp_mul(a.y, b.z), z2z2);
    const Fp s2 = fp_mul(fp_mul(b.y, a.z), z1z1);
    const Fp h = fp_sub(u2, u1);
    const Fp rr = fp_sub(s2, s1);
    if (fp_is_zero(h)) {
        if (fp_is_zero(rr)) return jac_dbl(a);
        return jac_inf();
    }
    const Fp i = fp_sqr(fp_dbl(h));
    const Fp j = fp_mul(h, i);
    const Fp r = fp_dbl(rr);
    const Fp v = fp_mul(u1, i);
    Jac o;
    o.x = fp_sub(fp_sub(fp_sqr(r), j), fp_dbl(v));
    o.y = fp_sub(fp_mul(r, fp_sub(v, o.x)), fp_dbl(fp_mul(s1, j)));
    o.z = fp_mul(fp_sub(fp_sub(fp_sqr(fp_add(a.z, b.z)), z1z1), z2z2), h);
    return o;
}

// the affine point (one inversion)
BK_HD Aff jac_to_aff(const Jac &a) {
    if (jac_is_inf(a)) return aff_inf();
    const Fp zi = fp_inv(a.z);
    const Fp zi2 = fp_sqr(zi);
    return Aff{fp_mul(a.x, zi2), fp_mul(fp_mul(a.y, zi), zi2)};
}

// pointG1.MarshalBinary: infinity is 64 zero bytes
BK_HD void aff_marshal(const Aff &a, uint8_t *out) {
    // (0, 0) out of Montgomery form is (0, 0): infinity needs no branch
    fp_to_bytes(fp_from_mont(a.x), out);
    fp_to_bytes(fp_from_mont(a.y), out + 32);
}

// pointG1.UnmarshalBinary: false for a coordinate >= p or a point off the
// curve; 64 zero bytes are infinity
BK_HD bool aff_unmarshal(const uint8_t *in, Aff *out) {
    const Fp x = fp_from_bytes(in), y = fp_from_bytes(in + 32);
    if (fp_geq_p(x) || fp_geq_p(y)) return false;
    out->x = fp_to_mont(x);
    out->y = fp_to_mont(y);
    if (fp_is_zero(x) && fp_is_zero(y)) return true;
    return aff_on_curve(*out);
}

// ---- scalars ----------------------------------------------------------------

// SetInt64(v) is v mod n >= 0, so v P = |v| (-P) for v < 0; |INT64_MIN| = 2^63
BK_HD uint64_t scalar_abs(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }

// The signed 4-bit windows of m: m = sum_{w < 16} digit(w) 16^w + top 16^16
// with digit(w) in [-8, 7] and top in {0, 1}: the nibbles of m + 0x88..8
constexpr int WINDOWS = 17;
constexpr uint64_t WINDOW_BIAS = 0x8888888888888888ull;
BK_HD int scalar_digit(uint64_t m, int w) {
    const uint64_t b = m + WINDOW_BIAS;
    if (w == 16) return b < m ? 1 : 0;
    return (int)((b >> (4 * w)) & 15u) - 8;
}

// v P by plain double-and-add on |v| (the baseline, and the host's reference)
BK_HD Jac jac_mul_i64(const Aff &p, int64_t v) {
    const Aff q = v < 0 ? aff_neg(p) : p;
    const uint64_t m = scalar_abs(v);
    Jac r = jac_inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 63; bit >= 0; --bit) {
        r = jac_dbl(r);
        if ((m >> bit) & 1u) r = jac_add_aff(r, q);
    }
    return r;
}

// The table of one key point: its multiples 1 .. 8, affine, 512 bytes
constexpr int TABLE = 8;

}  // namespace bn
}  // namespace bk
