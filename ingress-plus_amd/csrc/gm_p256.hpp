// gm_p256.hpp -- NIST P-256 arithmetic for ES256 (gm_jwt.inc: k_jwt_ec), shared by the device and by the host
// compiler, which builds each EC key's table with the very functions the kernel runs.
//
// A field element is eight 32-bit limbs, least significant first, in Montgomery form mod
//   p = 2^256 - 2^224 + 2^192 + 2^96 - 1        (x stands for x 2^256 mod p), always < p.
// p = -1 mod 2^32, so -1/p mod 2^32 = 1: the multiplier m of a reduction row is the accumulator's low limb
// itself, and since t_0 = m, (t + m p) / 2^32 = (t >> 32) + m (p + 1) / 2^32 = (t >> 32) + m 2^64 + m 2^160
// - m 2^192 + m 2^224: three adds and a subtract of m into a carry chain, no multiply.  A product is 64
// multiply-adds (v_mad_u64_u32: 32 x 32 + 64 bits) and those chains.  Every loop is over a constant range and
// unrolls, so every limb is a register of its own.  There is no dedicated squaring: see DESIGN.md.
// A scalar (mod the group order n) uses the generic row: m = t_0 * -1/n, 16 multiply-adds a row.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define GM_P256_FN __device__ __forceinline__
#else
#define GM_P256_FN __host__ __device__ inline
#endif

namespace p256 {

struct Fe { uint32_t v[8]; };

// (constants are functions of the limb index: in an unrolled loop each is a literal)
#define GM_P256_CONST(name, ...) \
    GM_P256_FN constexpr uint32_t name(uint32_t j) { constexpr uint32_t c[8] = {__VA_ARGS__}; return c[j]; }
GM_P256_CONST(P, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu)
GM_P256_CONST(ONE, 0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u)   // 2^256 mod p
GM_P256_CONST(RR, 0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u)    // 2^512 mod p
GM_P256_CONST(CB, 0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu, 0xf7212ed6u, 0xe5a220abu, 0x04874834u, 0xdc30061du)    // the curve's b
GM_P256_CONST(GX, 0x18a9143cu, 0x79e730d4u, 0x5fedb601u, 0x75ba95fcu, 0x77622510u, 0x79fb732bu, 0xa53755c6u, 0x18905f76u)
GM_P256_CONST(GY, 0xce95560au, 0xddf25357u, 0xba19e45cu, 0x8b4ab8e4u, 0xdd21f325u, 0xd2e88688u, 0x25885d85u, 0x8571ff18u)
GM_P256_CONST(N, 0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu)
GM_P256_CONST(N_ONE, 0x039cdaafu, 0x0c46353du, 0x58e8617bu, 0x43190552u, 0x00000000u, 0x00000000u, 0xffffffffu, 0x00000000u) // 2^256 mod n
GM_P256_CONST(N_RR, 0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu, 0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u)  // 2^512 mod n
#undef GM_P256_CONST
// -1/n mod 2^32, by Newton's iteration (each step doubles the correct low bits of 1/n)
GM_P256_FN constexpr uint32_t n0inv() { uint32_t x = 1; for (int i = 0; i < 5; i++) x *= 2u - N(0) * x; return 0u - x; }
static_assert(n0inv() == 0xee00bc4fu && (uint32_t)(N(0) * n0inv()) == 0xffffffffu, "-1/n mod 2^32");

// a - m: the borrow (1: a < m).  M is P or N.
#define GM_P256_BORROW(a, M, bw) \
    _Pragma("unroll") for (uint32_t j_ = 0; j_ < 8; j_++) bw = (uint32_t)(((uint64_t)(a).v[j_] - M(j_) - bw) >> 63);
GM_P256_FN bool lt_p(const Fe &a) { uint32_t bw = 0; GM_P256_BORROW(a, P, bw) return bw != 0; }
GM_P256_FN bool lt_n(const Fe &a) { uint32_t bw = 0; GM_P256_BORROW(a, N, bw) return bw != 0; }
GM_P256_FN uint32_t fe_or(const Fe &a) { uint32_t o = 0; for (uint32_t j = 0; j < 8; j++) o |= a.v[j]; return o; }
GM_P256_FN uint32_t fe_diff(const Fe &a, const Fe &b) { uint32_t o = 0; for (uint32_t j = 0; j < 8; j++) o |= a.v[j] ^ b.v[j]; return o; }
// c ? a : b by mask (written as a ?: the compiler turns the choice of whole elements into a branch and a private array)
GM_P256_FN Fe fe_sel(bool c, const Fe &a, const Fe &b) {
    const uint32_t m = 0u - (uint32_t)c;
    Fe r;
    for (uint32_t j = 0; j < 8; j++) r.v[j] = (a.v[j] & m) | (b.v[j] & ~m);
    return r;
}
GM_P256_FN Fe fe_one() { Fe r; for (uint32_t j = 0; j < 8; j++) r.v[j] = ONE(j); return r; }

// t (eight limbs and `top` above them, t < 2 m) reduced once: t - m if t >= m.  M is P or N.
#define GM_P256_REDUCE(t, top, M, r) \
    { uint32_t bw_ = 0; \
      _Pragma("unroll") for (uint32_t j_ = 0; j_ < 8; j_++) bw_ = (uint32_t)(((uint64_t)(t)[j_] - M(j_) - bw_) >> 63); \
      const uint32_t sub_ = ((top) | (bw_ ^ 1u)) ? 0xFFFFFFFFu : 0u; \
      bw_ = 0; \
      _Pragma("unroll") for (uint32_t j_ = 0; j_ < 8; j_++) { \
          const uint64_t d_ = (uint64_t)(t)[j_] - (M(j_) & sub_) - bw_; \
          (r).v[j_] = (uint32_t)d_; bw_ = (uint32_t)(d_ >> 63); } }

GM_P256_FN Fe fe_add(const Fe &a, const Fe &b) {
    uint32_t t[8];
    uint64_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { c = (uint64_t)a.v[j] + b.v[j] + (c >> 32); t[j] = (uint32_t)c; }
    Fe r;
    GM_P256_REDUCE(t, (uint32_t)(c >> 32), P, r)
    return r;
}
GM_P256_FN Fe fe_sub(const Fe &a, const Fe &b) {   // a - b, + p if that borrows
    uint32_t t[8], bw = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { const uint64_t d = (uint64_t)a.v[j] - b.v[j] - bw; t[j] = (uint32_t)d; bw = (uint32_t)(d >> 63); }
    const uint32_t add = bw ? 0xFFFFFFFFu : 0u;
    Fe r;
    uint64_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { c = (uint64_t)t[j] + (P(j) & add) + (c >> 32); r.v[j] = (uint32_t)c; }
    return r;
}

// a b / 2^256 mod p, for a < 2^256 and b < p: eight rows, each t += a_i b, then the reduction above, t one limb down
GM_P256_FN Fe fe_mul(const Fe &a, const Fe &b) {
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8 = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) { c = (uint64_t)a.v[i] * b.v[j] + t[j] + (c >> 32); t[j] = (uint32_t)c; }
        const uint64_t hi = (uint64_t)t8 + (c >> 32);   // limbs 8 and 9 (t < 2^290)
        const uint32_t m = t[0];
        t[0] = t[1]; t[1] = t[2];
        c = (uint64_t)t[3] + m; t[2] = (uint32_t)c;
        c = (uint64_t)t[4] + (c >> 32); t[3] = (uint32_t)c;
        c = (uint64_t)t[5] + (c >> 32); t[4] = (uint32_t)c;
        c = (uint64_t)t[6] + m + (c >> 32); t[5] = (uint32_t)c;
        int64_t s = (int64_t)(uint64_t)t[7] - (int64_t)(uint64_t)m + (int64_t)(c >> 32); t[6] = (uint32_t)s;
        s = (int64_t)hi + (int64_t)(uint64_t)m + (s >> 32); t[7] = (uint32_t)s;
        t8 = (uint32_t)((uint64_t)s >> 32);
    }
    Fe r;
    GM_P256_REDUCE(t, t8, P, r)
    return r;
}
GM_P256_FN Fe fe_sqr(const Fe &a) { return fe_mul(a, a); }

// a b / 2^256 mod n, for a < 2^256 and b < n (so a value leaves Montgomery form by a product with a plain one)
GM_P256_FN Fe sc_mul(const Fe &a, const Fe &b) {
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t8 = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        uint64_t x = 0, y = 0;
        uint32_t m = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            x = (uint64_t)a.v[i] * b.v[j] + t[j] + (x >> 32);
            if (j == 0) m = (uint32_t)x * n0inv();
            y = (uint64_t)m * N(j) + (uint32_t)x + (y >> 32);
            if (j) t[j - 1] = (uint32_t)y;
        }
        const uint64_t z = (uint64_t)t8 + (x >> 32) + (y >> 32);
        t[7] = (uint32_t)z; t8 = (uint32_t)(z >> 32);
    }
    Fe r;
    GM_P256_REDUCE(t, t8, N, r)
    return r;
}
GM_P256_FN Fe sc_sqrn(Fe a, uint32_t k) {
#pragma unroll 1
    for (uint32_t i = 0; i < k; i++) a = sc_mul(a, a);
    return a;
}
// 1/s mod n in Montgomery form, of s in Montgomery form: s^(n - 2) by a fixed chain -- the exponent's top 128
// bits are FFFFFFFF 00000000 FFFFFFFF FFFFFFFF, runs of 32 ones (x^(2^32 - 1) by doubling the run length), its
// low 128 bits go bit by bit.  The exponent is a constant: every branch is uniform.
GM_P256_FN Fe sc_inv(const Fe &s) {
    Fe r = s;   // x^(2^k - 1) for k = 1, 2, 4, 8, 16, 32
#pragma unroll 1
    for (uint32_t k = 1; k < 32; k *= 2) r = sc_mul(sc_sqrn(r, k), r);
    Fe y = sc_mul(sc_sqrn(r, 64), r);
    y = sc_mul(sc_sqrn(y, 32), r);
#pragma unroll 1
    for (int i = 127; i >= 0; i--) {
        const uint32_t w = i >= 96 ? N(3) : i >= 64 ? N(2) : i >= 32 ? N(1) : N(0) - 2u;
        y = sc_mul(y, y);
        if (w >> (i & 31) & 1) y = sc_mul(y, s);
    }
    return y;
}

// A point in Jacobian coordinates (x = X / Z^2, y = Y / Z^3); Z = 0: the point at infinity.
struct Jac { Fe X, Y, Z; };

// 2 P (a = -3: 3 M + 5 S).  Z = 0 gives Z = 0, and the curve has no point with Y = 0.
GM_P256_FN Jac jac_dbl(const Jac &p) {
    const Fe delta = fe_sqr(p.Z), gamma = fe_sqr(p.Y), beta = fe_mul(p.X, gamma);
    const Fe h = fe_mul(fe_sub(p.X, delta), fe_add(p.X, delta));
    const Fe alpha = fe_add(fe_add(h, h), h);
    const Fe b2 = fe_add(beta, beta), b4 = fe_add(b2, b2);
    Jac r;
    r.X = fe_sub(fe_sqr(alpha), fe_add(b4, b4));
    r.Z = fe_sub(fe_sub(fe_sqr(fe_add(p.Y, p.Z)), gamma), delta);
    Fe g2 = fe_sqr(gamma);
    g2 = fe_add(g2, g2); g2 = fe_add(g2, g2); g2 = fe_add(g2, g2);
    r.Y = fe_sub(fe_mul(alpha, fe_sub(b4, r.X)), g2);
    return r;
}

// P + (x, y), the addend affine and not at infinity (8 M + 3 S), every case:
//   P at infinity: the addend.  P = the addend (H = 0 and r = 0): 2 P, by jac_dbl under a branch that is all but
//   never taken.  P = -(the addend) (H = 0, r != 0): Z3 = Z1 H = 0, the point at infinity, as the formula gives it.
GM_P256_FN Jac jac_madd(const Jac &p, const Fe &x, const Fe &y) {
    const Fe zz = fe_sqr(p.Z), u2 = fe_mul(x, zz), s2 = fe_mul(y, fe_mul(p.Z, zz));
    const Fe h = fe_sub(u2, p.X), r = fe_sub(s2, p.Y);
    const Fe hh = fe_sqr(h), hhh = fe_mul(h, hh), v = fe_mul(p.X, hh);
    Jac q;
    q.X = fe_sub(fe_sub(fe_sqr(r), hhh), fe_add(v, v));
    q.Y = fe_sub(fe_mul(r, fe_sub(v, q.X)), fe_mul(p.Y, hhh));
    q.Z = fe_mul(p.Z, h);
    const bool inf = fe_or(p.Z) == 0;
    if (!inf && (fe_or(h) | fe_or(r)) == 0) q = jac_dbl(p);
    q.X = fe_sel(inf, x, q.X); q.Y = fe_sel(inf, y, q.Y); q.Z = fe_sel(inf, fe_one(), q.Z);
    return q;
}

// A key's table (gm_tables.hpp DJwk): entry 4 i + j - 1 is the affine point i G + j Q, i, j in 0 .. 3 not both 0,
// x then y, sixteen words; no entry is the point at infinity (the compiler refuses such a key).
constexpr uint32_t TABLE_ENTRIES = 15, TABLE_WORDS = TABLE_ENTRIES * 16;
struct alignas(16) Quad { uint32_t a, b, c, d; };   // (one dwordx4 load)

// ECDSA: whether (r, s) signs the digest e (any value below 2^256) under the key whose table is T.
//   1 <= r, s < n;  w = 1 / s, u1 = e w, u2 = r w (mod n);  R = u1 G + u2 Q by Shamir's trick over joint 2-bit
//   windows, most significant first: 128 steps of two doublings and one mixed addition of T[i][j], the (0, 0)
//   window's addition computed on entry 0 and dropped by select.  R at infinity (Z = 0) is refused before the
//   compare; x_R mod n = r is tested without an inversion as r Z^2 = X or, if r + n < p, (r + n) Z^2 = X.
GM_P256_FN bool ecdsa_verify(const Fe &e, const Fe &r, const Fe &s, const uint32_t *__restrict__ T) {
    const bool range = fe_or(r) != 0 && fe_or(s) != 0 && lt_n(r) && lt_n(s);
    Fe c;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) c.v[j] = N_RR(j);
    const Fe w = sc_inv(sc_mul(s, c));
    Fe u1 = sc_mul(e, w), u2 = sc_mul(r, w);
    Jac acc;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) acc.X.v[j] = acc.Y.v[j] = acc.Z.v[j] = 0;
    const Quad *Tq = reinterpret_cast<const Quad *>(T);
#pragma unroll 1
    for (uint32_t k = 0; k < 128; k++) {
        const uint32_t idx = (u1.v[7] >> 30) * 4 + (u2.v[7] >> 30);
#pragma unroll
        for (uint32_t j = 7; j > 0; j--) {
            u1.v[j] = u1.v[j] << 2 | u1.v[j - 1] >> 30;
            u2.v[j] = u2.v[j] << 2 | u2.v[j - 1] >> 30;
        }
        u1.v[0] <<= 2; u2.v[0] <<= 2;
        const Quad *E = Tq + 4 * (idx ? idx - 1 : 0u);
        const Quad x0 = E[0], x1 = E[1], y0 = E[2], y1 = E[3];
        const Fe x = {{x0.a, x0.b, x0.c, x0.d, x1.a, x1.b, x1.c, x1.d}}, y = {{y0.a, y0.b, y0.c, y0.d, y1.a, y1.b, y1.c, y1.d}};
        acc = jac_dbl(jac_dbl(acc));
        const Jac q = jac_madd(acc, x, y);
        acc.X = fe_sel(idx != 0, q.X, acc.X); acc.Y = fe_sel(idx != 0, q.Y, acc.Y); acc.Z = fe_sel(idx != 0, q.Z, acc.Z);
    }
    const bool finite = fe_or(acc.Z) != 0;
    const Fe zz = fe_sqr(acc.Z);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) c.v[j] = RR(j);
    Fe rn;
    uint64_t cy = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { cy = (uint64_t)r.v[j] + N(j) + (cy >> 32); rn.v[j] = (uint32_t)cy; }
    const bool second = (cy >> 32) == 0 && lt_p(rn);
    const uint32_t d1 = fe_diff(fe_mul(fe_mul(r, c), zz), acc.X), d2 = fe_diff(fe_mul(fe_mul(rn, c), zz), acc.X);
    return ((uint32_t)range & (uint32_t)finite & ((uint32_t)(d1 == 0) | ((uint32_t)second & (uint32_t)(d2 == 0)))) != 0;
}

}   // namespace p256
