// The field mod q = 2^255 - 19 (curves/curve25519/affine_point.rs:39-44, BASE_FIELD) as inline host/device math.
// Replaces the reference's PrimeFieldElem over a BigUint (`*` then `%`, field/prime_field_elem.rs).
//
// Shipped form: eight 32-bit limbs, a value is ANY integer below 2^256 (two or three representatives per residue).  q is a pseudo-Mersenne prime:
// 2^256 = 38 (mod q), so a product is the 8 x 8 product scan (64 v_mad_u64_u32 with the column's third word, as in fp.h) and ONE fold
// low + 38 * high — no Montgomery step, against the 2 N^2 + N = 136 multiply-adds of the generic scan.  A dedicated squaring does not win with
// full 32-bit limbs (fp.h, fp_sqr), so the square is the product.  Values are made canonical only where bytes leave (fe_to_words) or are compared.
//
// -DZKT_FE25519_MONT builds the SAME interface over the generic Montgomery Fp<Fe25519C> of fp.h: the A/B baseline of profiles/ed25519_timing.md.
#pragma once
#include "fp.h"
#include "ed25519_constants.h"

namespace zkt {

#if defined(ZKT_FE25519_MONT)

typedef Fp<Fe25519C> Fe;
ZKT_HD Fe fe_from_words(const uint32_t* w) { return fp_from_words<Fe25519C>(w); }               // any value below 2^256 (< 3q: two conditional subtractions)
ZKT_HD void fe_to_words(const Fe& a, uint32_t* w) { fp_to_words(a, w); }
ZKT_HD Fe fe_mul(const Fe& a, const Fe& b) { return fp_mul(a, b); }
ZKT_HD Fe fe_sqr(const Fe& a) { return fp_mul(a, a); }
ZKT_HD Fe fe_add(const Fe& a, const Fe& b) { return fp_add(a, b); }
ZKT_HD Fe fe_sub(const Fe& a, const Fe& b) { return fp_sub(a, b); }
ZKT_HD Fe fe_neg(const Fe& a) { return fp_neg(a); }
ZKT_HD bool fe_is_zero(const Fe& a) { return fp_is_zero(a); }
ZKT_HD bool fe_eq(const Fe& a, const Fe& b) { return fp_eq(a, b); }
ZKT_HD Fe fe_zero() { return fp_zero<Fe25519C>(); }
ZKT_HD Fe fe_one() { return fp_one<Fe25519C>(); }
// raw limbs in tables written by this same build
ZKT_HD Fe fe_ld_raw(const uint32_t* p, int stride = 1) { Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = p[i * stride]; return r; }
ZKT_HD void fe_st_raw(uint32_t* p, const Fe& a, int stride = 1) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i * stride] = a.v[i]; }

#else

struct Fe { uint32_t v[8]; };

ZKT_HD Fe fe_zero() { Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = 0; return r; }
ZKT_HD Fe fe_one() { Fe r = fe_zero(); r.v[0] = 1; return r; }
ZKT_HD Fe fe_from_words(const uint32_t* w) { Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = w[i]; return r; }
ZKT_HD Fe fe_ld_raw(const uint32_t* p, int stride = 1) { Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = p[i * stride]; return r; }
ZKT_HD void fe_st_raw(uint32_t* p, const Fe& a, int stride = 1) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i * stride] = a.v[i]; }

// r + cy * 2^256 -> the same residue below 2^256 (cy <= 38): 2^256 = 38.  A second carry leaves r < 38 * 39, so the third step cannot carry.
ZKT_HD void fe_fold_carry(Fe& r, uint32_t cy) {
  uint32_t c = 0;
  r.v[0] = addc(r.v[0], cy * 38u, c);
#pragma unroll
  for (int i = 1; i < 8; ++i) r.v[i] = addc(r.v[i], 0u, c);
  r.v[0] += c * 38u;
}
ZKT_HD Fe fe_add(const Fe& a, const Fe& b) {
  Fe r; uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = addc(a.v[i], b.v[i], c);
  fe_fold_carry(r, c);
  return r;
}
// a - b: a borrow means the limbs hold a - b + 2^256 = (a - b) + 38; a second borrow (the limbs were below 38) the same again, and then the limbs are
// within 38 of 2^256, so the last step cannot borrow
ZKT_HD Fe fe_sub(const Fe& a, const Fe& b) {
  Fe r; uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = subb(a.v[i], b.v[i], bw);
  uint32_t b2 = 0;
  r.v[0] = subb(r.v[0], bw * 38u, b2);
#pragma unroll
  for (int i = 1; i < 8; ++i) r.v[i] = subb(r.v[i], 0u, b2);
  r.v[0] -= b2 * 38u;
  return r;
}
ZKT_HD Fe fe_neg(const Fe& a) { return fe_sub(fe_zero(), a); }

// the product scan: column k sums a_i b_(k-i) into a 96-bit accumulator (fp.h, mac), then low + 38 * high with the constant in an SGPR
ZKT_HD Fe fe_mul(const Fe& a, const Fe& b) {
  uint32_t t[16]; uint64_t lo = 0; uint32_t hi = 0;
#pragma unroll
  for (int k = 0; k < 15; ++k) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { if (k - i >= 0 && k - i < 8) mac(lo, hi, a.v[i], b.v[k - i]); }
    t[k] = (uint32_t)lo; lo = (lo >> 32) | ((uint64_t)hi << 32); hi = 0;
  }
  t[15] = (uint32_t)lo;
  Fe r; uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += t[i]; uint32_t h = 0;
    mac_k(c, h, t[8 + i], 38u);                         // c < 2^32 + 2^32 + 38 * 2^32: the third word stays 0
    r.v[i] = (uint32_t)c; c >>= 32;
  }
  fe_fold_carry(r, (uint32_t)c);                        // c <= 38
  return r;
}
ZKT_HD Fe fe_sqr(const Fe& a) { return fe_mul(a, a); }

// the canonical residue: bit 255 folds to 19 (2^255 = 19), which leaves a value below 2^255 + 19 < 2q; then one conditional subtraction of q
ZKT_HD void fe_to_words(const Fe& a, uint32_t* w) {
  uint32_t v[8], c = 0;
  const uint32_t top = a.v[7] >> 31;
  v[0] = addc(a.v[0], top * 19u, c);
#pragma unroll
  for (int i = 1; i < 7; ++i) v[i] = addc(a.v[i], 0u, c);
  v[7] = (a.v[7] & 0x7fffffffu) + c;
  uint32_t s[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = subb(v[i], ed25519_q_word(i), bw);
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = bw ? v[i] : s[i];
}
ZKT_HD bool fe_is_zero(const Fe& a) {
  uint32_t w[8], o = 0;
  fe_to_words(a, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= w[i];
  return o == 0;
}
ZKT_HD bool fe_eq(const Fe& a, const Fe& b) { return fe_is_zero(fe_sub(a, b)); }

#endif  // ZKT_FE25519_MONT

#define ZKT_FE_CONST(name, wordfn) ZKT_HD Fe name() { uint32_t w[8]; _Pragma("unroll") for (int i = 0; i < 8; ++i) w[i] = wordfn(i); return fe_from_words(w); }
ZKT_FE_CONST(fe_d, ed25519_d_word)
ZKT_FE_CONST(fe_2d, ed25519_2d_word)
ZKT_FE_CONST(fe_sqrtm1, ed25519_sqrtm1_word)
#undef ZKT_FE_CONST

// parity of the canonical residue (get_parity, affine_point.rs:75-77)
ZKT_HD uint32_t fe_parity(const Fe& a) { uint32_t w[8]; fe_to_words(a, w); return w[0] & 1u; }
ZKT_HD Fe fe_sqn(Fe a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) a = fe_sqr(a);
  return a;
}
// z^(2^250 - 1) and z^11: the shared head of the two addition chains below (11 products, 249 squarings)
ZKT_HD Fe fe_pow_2_250_m1(const Fe& z, Fe& z11) {
  const Fe z2 = fe_sqr(z), z9 = fe_mul(fe_sqn(z2, 2), z);
  z11 = fe_mul(z9, z2);
  const Fe t5 = fe_mul(fe_sqr(z11), z9);                          // 2^5 - 1
  const Fe t10 = fe_mul(fe_sqn(t5, 5), t5);                       // 2^10 - 1
  const Fe t20 = fe_mul(fe_sqn(t10, 10), t10);
  const Fe t40 = fe_mul(fe_sqn(t20, 20), t20);
  const Fe t50 = fe_mul(fe_sqn(t40, 10), t10);
  const Fe t100 = fe_mul(fe_sqn(t50, 50), t50);
  const Fe t200 = fe_mul(fe_sqn(t100, 100), t100);
  return fe_mul(fe_sqn(t200, 50), t50);
}
// z^(q-2) = z^(2^255 - 21): the inverse, 0 for z = 0
ZKT_HD Fe fe_inv(const Fe& z) { Fe z11; const Fe t = fe_pow_2_250_m1(z, z11); return fe_mul(fe_sqn(t, 5), z11); }
// z^((q-5)/8) = z^(2^252 - 3)
ZKT_HD Fe fe_pow_q58(const Fe& z) { Fe z11; const Fe t = fe_pow_2_250_m1(z, z11); return fe_mul(fe_sqn(t, 2), z); }

// recover_x's root (affine_point.rs:83-99) for xx = u / v, v != 0: x = xx^((q+3)/8), times I if x^2 != xx — and NO further test, as there.
// One power: u v^3 (u v^7)^((q-5)/8) = u^((q+3)/8) v^((7q-11)/8) = (u/v)^((q+3)/8), since v^(q-1) = 1.  Returns x^2 == xx for the x handed back.
ZKT_HD bool fe_sqrt_ratio(const Fe& u, const Fe& v, Fe& x) {
  const Fe v3 = fe_mul(fe_sqr(v), v), v7 = fe_mul(fe_sqr(v3), v);
  x = fe_mul(fe_mul(u, v3), fe_pow_q58(fe_mul(u, v7)));
  if (fe_eq(fe_mul(v, fe_sqr(x)), u)) return true;
  x = fe_mul(x, fe_sqrtm1());
  return fe_eq(fe_mul(v, fe_sqr(x)), u);
}

}  // namespace zkt
