// Ed25519 over SHA-512, one key / one signature per caller (per lane on the device), as inline host/device math over fe25519.h and sha512.h.
//   decode_point / encode_point   src/building_block/curves/curve25519/ed25519_sha512.rs:64-98, recover_x affine_point.rs:83-104
//   gen_pub_key                   ed25519_sha512.rs:115-125
//   sign                          ed25519_sha512.rs:127-158
//   verify                        ed25519_sha512.rs:160-186
// The reference adds affine points with the Edwards law (affine_point.rs:119-143, two divisions per addition) along an LSB-first chain that starts from
// the rational point (0, 1) (macros.rs:1-32).  -1 is a square and d is not, so the law is complete on the curve's points: there the result does not depend
// on the chain, and this file uses extended coordinates (X : Y : Z : T), a = -1, with the unified addition on (Y-X, Y+X, 2dT, Z) entries and the
// dedicated doubling (Hisil-Wong-Carter-Dawson 2008), both complete on the curve as well.
// Integers mod l are eight little-endian 32-bit words; `btab` is the base point's comb table: entry [w * 15 + d - 1] = d * 16^w * B as (y-x, y+x, 2dxy), raw limbs.
#pragma once
#include "fe25519.h"
#include "sha512.h"

namespace zkt {

// ---- bytes <-> little-endian words: word accesses where the address allows, bytes otherwise (a caller's device arrays need no alignment) ----------------
ZKT_HD void ld_le_words(const uint8_t* p, uint32_t* w, int n) {
  if ((((uintptr_t)p) & 3u) == 0) { for (int i = 0; i < n; ++i) w[i] = ((const uint32_t*)p)[i]; return; }
  for (int i = 0; i < n; ++i) w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
}
ZKT_HD void st_le_words(uint8_t* p, const uint32_t* w, int n) {
  if ((((uintptr_t)p) & 3u) == 0) { for (int i = 0; i < n; ++i) ((uint32_t*)p)[i] = w[i]; return; }
  for (int i = 0; i < n; ++i) { p[4 * i] = (uint8_t)w[i]; p[4 * i + 1] = (uint8_t)(w[i] >> 8); p[4 * i + 2] = (uint8_t)(w[i] >> 16); p[4 * i + 3] = (uint8_t)(w[i] >> 24); }
}
// 32 bytes as little-endian words -> the four big-endian 64-bit words SHA-512 reads them as
ZKT_HD void sha_words_of_le(const uint32_t w[8], uint64_t o[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = ((uint64_t)__builtin_bswap32(w[2 * i]) << 32) | __builtin_bswap32(w[2 * i + 1]);
}
// the digest (state words big-endian) read as a 512-bit little-endian integer (BigUint::from_bytes_le, ed25519_sha512.rs:141, :172)
ZKT_HD void le_words_of_state(const uint64_t h[8], uint32_t o[16]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { o[2 * i] = __builtin_bswap32((uint32_t)(h[i] >> 32)); o[2 * i + 1] = __builtin_bswap32((uint32_t)h[i]); }
}

// ---- integers mod l = 2^252 + c (affine_point.rs:46-51, CURVE_GROUP): plain carry chains ------------------------------------------------------
template <int NA, int NB> ZKT_HD void mp_mul(const uint32_t* a, const uint32_t* b, uint32_t* o) {      // o: NA + NB words
  uint64_t lo = 0; uint32_t hi = 0;
#pragma unroll
  for (int k = 0; k < NA + NB - 1; ++k) {
#pragma unroll
    for (int i = 0; i < NA; ++i) { if (k - i >= 0 && k - i < NB) mac(lo, hi, a[i], b[k - i]); }
    o[k] = (uint32_t)lo; lo = (lo >> 32) | ((uint64_t)hi << 32); hi = 0;
  }
  o[NA + NB - 1] = (uint32_t)lo;
}
// o = in >> 252 (NOUT words), lo = in mod 2^252 (8 words)
template <int NIN, int NOUT> ZKT_HD void sc_split252(const uint32_t* in, uint32_t* lo, uint32_t* o) {
#pragma unroll
  for (int i = 0; i < 8; ++i) lo[i] = i < NIN ? in[i] : 0u;
  lo[7] &= 0x0fffffffu;
#pragma unroll
  for (int i = 0; i < NOUT; ++i) o[i] = (i + 7 < NIN ? in[i + 7] >> 28 : 0u) | (i + 8 < NIN ? in[i + 8] << 4 : 0u);
}
// a -= m << sh if that leaves a >= 0 (a, m: 8 words)
ZKT_HD void sc_cond_sub_l(uint32_t a[8], int sh) {
  uint32_t s[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t m = sh ? ((ed25519_l_word(i) << sh) | (i ? ed25519_l_word(i - 1) >> (32 - sh) : 0u)) : ed25519_l_word(i);
    s[i] = subb(a[i], m, bw);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = bw ? a[i] : s[i];
}
ZKT_HD bool sc_below_l(const uint32_t a[8]) {
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) (void)subb(a[i], ed25519_l_word(i), bw);
  return bw != 0;
}
// x mod l for any 512-bit x.  2^252 = -c (mod l), c of 125 bits: with x = x0 + 2^252 h0, h0 c = p1 = p1' + 2^252 h1 (h1 < 2^133), h1 c = p2 = p2' + 2^252 h2
// (h2 < 2^6), p3 = h2 c < 2^131:  x = x0 - p1' + p2' - p3 (mod l).  Every term is below 2^252 < l, so t = x0 + p2' + 2l - p1' - p3 lies in (0, 4l).
ZKT_HD void sc_reduce512(const uint32_t x[16], uint32_t r[8]) {
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = ed25519_lc_word(i);
  uint32_t x0[8], h0[9], p1[13], q1[8], h1[5], p2[9], q2[8], h2[1], p3[5];
  sc_split252<16, 9>(x, x0, h0);
  mp_mul<9, 4>(h0, c, p1);
  sc_split252<13, 5>(p1, q1, h1);
  mp_mul<5, 4>(h1, c, p2);
  sc_split252<9, 1>(p2, q2, h2);
  mp_mul<1, 4>(h2, c, p3);
  uint32_t cy = 0, cy2 = 0, bw = 0, bw2 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t l2 = (ed25519_l_word(i) << 1) | (i ? ed25519_l_word(i - 1) >> 31 : 0u);
    uint32_t t = addc(x0[i], q2[i], cy);
    t = addc(t, l2, cy2);
    t = subb(t, q1[i], bw);
    r[i] = subb(t, i < 5 ? p3[i] : 0u, bw2);
  }
  sc_cond_sub_l(r, 1);
  sc_cond_sub_l(r, 0);
}
// (a b + c) mod l for any 256-bit a, b, c: a b + c < 2^512
ZKT_HD void sc_muladd(const uint32_t a[8], const uint32_t b[8], const uint32_t c[8], uint32_t r[8]) {
  uint32_t p[16], cy = 0;
  mp_mul<8, 8>(a, b, p);
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = addc(p[i], i < 8 ? c[i] : 0u, cy);
  sc_reduce512(p, r);
}
// 8 a mod l for any 256-bit a (f_l.elem(&(S * 8u8)), ed25519_sha512.rs:177)
ZKT_HD void sc_mul8(const uint32_t a[8], uint32_t r[8]) {
  uint32_t p[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = (i < 8 ? a[i] << 3 : 0u) | (i >= 1 && i <= 8 ? a[i - 1] >> 29 : 0u);
  sc_reduce512(p, r);
}

// ---- the group ------------------------------------------------------------------------------------------------------------------------------
struct Ge { Fe X, Y, Z, T; };                   // x = X/Z, y = Y/Z, T = XY/Z
struct GeCached { Fe ymx, ypx, t2d, Z; };       // (Y-X, Y+X, 2dT, Z)
static constexpr int ED_PRE_WORDS = 24;         // one comb entry: (y-x, y+x, 2dxy), Z = 1
static constexpr int ED_COMB_ENTRIES = 64 * 15;
static constexpr int ED_CW = 32;                // words of one GeCached
#if !defined(ZKT_ED25519_WIN)
#define ZKT_ED25519_WIN 4                       // window width of the [8k](-A) chain
#endif
static constexpr int ED_WIN = ZKT_ED25519_WIN;
static constexpr int ED_TAB = (1 << ED_WIN) - 1;

ZKT_HD Ge ge_neutral() { Ge r; r.X = fe_zero(); r.Y = fe_one(); r.Z = fe_one(); r.T = fe_zero(); return r; }     // AffinePoint::zero(), affine_point.rs:167-173
ZKT_HD Ge ge_from_affine(const Fe& x, const Fe& y) { Ge r; r.X = x; r.Y = y; r.Z = fe_one(); r.T = fe_mul(x, y); return r; }
ZKT_HD GeCached ge_to_cached(const Ge& p) { GeCached c; c.ymx = fe_sub(p.Y, p.X); c.ypx = fe_add(p.Y, p.X); c.t2d = fe_mul(p.T, fe_2d()); c.Z = p.Z; return c; }
// dbl-2008-hwcd with a = -1: 4 squarings + 3 products, + 1 for T (which only an addition reads)
template <bool WITH_T> ZKT_HD Ge ge_dbl(const Ge& p) {
  const Fe A = fe_sqr(p.X), B = fe_sqr(p.Y), Z2 = fe_sqr(p.Z), C = fe_add(Z2, Z2);
  const Fe E = fe_sub(fe_sub(fe_sqr(fe_add(p.X, p.Y)), A), B), G = fe_sub(B, A), F = fe_sub(G, C), H = fe_neg(fe_add(A, B));
  Ge r; r.X = fe_mul(E, F); r.Y = fe_mul(G, H); r.Z = fe_mul(F, G);
  if (WITH_T) r.T = fe_mul(E, H); else r.T = fe_zero();
  return r;
}
// add-2008-hwcd-3 with k = 2d folded into the entry: 8 products (7 when the entry is affine)
ZKT_HD Ge ge_add_parts(const Ge& p, const Fe& ymx, const Fe& ypx, const Fe& t2d, const Fe& D) {
  const Fe A = fe_mul(fe_sub(p.Y, p.X), ymx), B = fe_mul(fe_add(p.Y, p.X), ypx), C = fe_mul(p.T, t2d);
  const Fe E = fe_sub(B, A), F = fe_sub(D, C), G = fe_add(D, C), H = fe_add(B, A);
  Ge r; r.X = fe_mul(E, F); r.Y = fe_mul(G, H); r.T = fe_mul(E, H); r.Z = fe_mul(F, G);
  return r;
}
ZKT_HD Ge ge_add(const Ge& p, const GeCached& q) { const Fe zz = fe_mul(p.Z, q.Z); return ge_add_parts(p, q.ymx, q.ypx, q.t2d, fe_add(zz, zz)); }
ZKT_HD Ge ge_madd(const Ge& p, const uint32_t* e) { return ge_add_parts(p, fe_ld_raw(e), fe_ld_raw(e + 8), fe_ld_raw(e + 16), fe_add(p.Z, p.Z)); }
// the neutral element: x = 0 and y = 1
ZKT_HD bool ge_is_neutral(const Ge& p) { return fe_is_zero(p.X) && fe_eq(p.Y, p.Z); }

template <int STRIDE> ZKT_HD void ge_st_cached(uint32_t* p, const GeCached& c) {
  fe_st_raw(p, c.ymx, STRIDE); fe_st_raw(p + 8 * STRIDE, c.ypx, STRIDE); fe_st_raw(p + 16 * STRIDE, c.t2d, STRIDE); fe_st_raw(p + 24 * STRIDE, c.Z, STRIDE);
}
template <int STRIDE> ZKT_HD GeCached ge_ld_cached(const uint32_t* p) {
  GeCached c; c.ymx = fe_ld_raw(p, STRIDE); c.ypx = fe_ld_raw(p + 8 * STRIDE, STRIDE); c.t2d = fe_ld_raw(p + 16 * STRIDE, STRIDE); c.Z = fe_ld_raw(p + 24 * STRIDE, STRIDE);
  return c;
}

// 4-bit digit w of an 8-word integer, without a dynamically indexed register array
ZKT_HD uint32_t sc_digit4(const uint32_t k[8], int w) {
  uint32_t kw = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) kw = (j == (w >> 3)) ? k[j] : kw;
  return (kw >> ((w & 7) * 4)) & 15u;
}
// acc + k * B from the comb table: at most 64 mixed additions, no doubling; k is any 256-bit integer
ZKT_HD Ge ed25519_add_base_multiple(Ge acc, const uint32_t* btab, const uint32_t k[8]) {
#pragma unroll 1
  for (int w = 0; w < 64; ++w) {
    const uint32_t d = sc_digit4(k, w);
    if (d) acc = ge_madd(acc, btab + ((size_t)w * 15 + d - 1) * ED_PRE_WORDS);
  }
  return acc;
}
// entry t = w * 15 + d - 1 of the comb table: d * 16^w * B, normalised (one inversion)
ZKT_HD void ed25519_comb_entry(int t, uint32_t* out) {
  const int w = t / 15, d = t % 15 + 1;
  uint32_t bx[8], by[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { bx[i] = ed25519_bx_word(i); by[i] = ed25519_by_word(i); }
  Ge p = ge_from_affine(fe_from_words(bx), fe_from_words(by));
#pragma unroll 1
  for (int i = 0; i < 4 * w; ++i) p = ge_dbl<true>(p);
  const GeCached c = ge_to_cached(p);
  Ge q = p;
#pragma unroll 1
  for (int i = 1; i < d; ++i) q = ge_add(q, c);
  const Fe zi = fe_inv(q.Z), x = fe_mul(q.X, zi), y = fe_mul(q.Y, zi);
  fe_st_raw(out, fe_sub(y, x)); fe_st_raw(out + 8, fe_add(y, x)); fe_st_raw(out + 16, fe_mul(fe_mul(x, y), fe_2d()));
}

// decode_point (ed25519_sha512.rs:85-98): bit 255 is the wanted parity of x, the other 255 bits are y, taken mod q (y >= q is accepted);
// x = recover_x(y).  Returns whether (x, y) is on the curve; x is the reference's value bit for bit either way.
ZKT_HD bool ed25519_decode_one(const uint32_t enc[8], Fe& x, Fe& y) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = enc[i];
  const uint32_t sign = w[7] >> 31;
  w[7] &= 0x7fffffffu;
  y = fe_from_words(w);
  const Fe yy = fe_sqr(y), u = fe_sub(yy, fe_one()), v = fe_add(fe_mul(fe_d(), yy), fe_one());      // xx = (y^2 - 1) / (d y^2 + 1); d y^2 + 1 != 0: -1/d is no square
  const bool on = fe_sqrt_ratio(u, v, x);
  if (fe_parity(x) != sign) x = fe_neg(x);                   // x = 0 with the sign bit set stays 0 (affine_point.rs:100-103)
  return on;
}
// encode_point (:64-83) of an affine point: the canonical y with the parity of the canonical x in bit 255
ZKT_HD void ed25519_encode_affine(const Fe& x, const Fe& y, uint32_t enc[8]) {
  fe_to_words(y, enc);
  enc[7] |= fe_parity(x) << 31;
}
ZKT_HD void ed25519_encode(const Ge& p, uint32_t enc[8]) {
  const Fe zi = fe_inv(p.Z);
  ed25519_encode_affine(fe_mul(p.X, zi), fe_mul(p.Y, zi), enc);
}

// H(prv) -> the pruned scalar s (gen_s, :100-113) and the prefix as SHA-512 words (digest[32..64], :134)
ZKT_HD void ed25519_expand_key(const uint8_t* prv, uint32_t s[8], uint64_t prefix[4]) {
  uint64_t h[8]; uint32_t dw[16];
  sha512_words<0>(nullptr, prv, 32, h);
  le_words_of_state(h, dw);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = dw[i];
  s[0] &= 0xfffffff8u; s[7] &= 0x7fffffffu; s[7] |= 0x40000000u;
#pragma unroll
  for (int i = 0; i < 4; ++i) prefix[i] = h[4 + i];
}
// encode(B * base_field().elem(s)) (:121-123, :136-137): the multiplier is s mod q, NOT s — it differs from s for s = 2^255 - 16 and 2^255 - 8 only
// (3 and 11), which no private key reaches; one conditional subtraction reproduces it.  s: any integer below 2^255 + 2^254.
ZKT_HD void ed25519_pub_from_scalar(const uint32_t s[8], const uint32_t* btab, uint32_t enc[8]) {
  uint32_t m[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = subb(s[i], ed25519_q_word(i), bw);
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = bw ? s[i] : m[i];
  ed25519_encode(ed25519_add_base_multiple(ge_neutral(), btab, m), enc);
}
// gen_pub_key (:115-125)
ZKT_HD void ed25519_public_key_one(const uint8_t* prv, const uint32_t* btab, uint8_t* pub) {
  uint32_t s[8], enc[8]; uint64_t prefix[4];
  ed25519_expand_key(prv, s, prefix);
  ed25519_pub_from_scalar(s, btab, enc);
  st_le_words(pub, enc, 8);
}
// the tail of sign (:139-157) from the expanded key: r = H(prefix ‖ msg) mod l, R = enc(B r), k = H(R ‖ A ‖ msg) mod l, S = (r + k s) mod l with the UNREDUCED s
ZKT_HD void ed25519_sign_expanded(const uint8_t* msg, uint64_t len, const uint32_t s[8], const uint64_t prefix[4], const uint32_t* btab, uint8_t* sig) {
  uint32_t A[8], R[8], r[8], k[8], S[8], dw[16]; uint64_t h[8], ra[8];
  ed25519_pub_from_scalar(s, btab, A);
  sha512_words<4>(prefix, msg, len, h);
  le_words_of_state(h, dw);
  sc_reduce512(dw, r);
  ed25519_encode(ed25519_add_base_multiple(ge_neutral(), btab, r), R);      // r < l < q: elem(r) = r
  sha_words_of_le(R, ra); sha_words_of_le(A, ra + 4);
  sha512_words<8>(ra, msg, len, h);
  le_words_of_state(h, dw);
  sc_reduce512(dw, k);
  sc_muladd(k, s, r, S);
  st_le_words(sig, R, 8); st_le_words(sig + 32, S, 8);
}
// sign (:127-158); deterministic
ZKT_HD void ed25519_sign_one(const uint8_t* msg, uint64_t len, const uint8_t* prv, const uint32_t* btab, uint8_t* sig) {
  uint32_t s[8]; uint64_t prefix[4];
  ed25519_expand_key(prv, s, prefix);
  ed25519_sign_expanded(msg, len, s, prefix, btab, sig);
}

// verify (:160-186) for one signature.  In the reference's order: S >= l rejects (:165-167); R is decoded and RE-ENCODED (:168-169: canonical y, the
// actual parity of x) and that encoding is hashed with the key's bytes AS GIVEN (:170); lhs = B (8S mod l), rhs = R 8 + A (8k mod l) with the full points
// (:176-185).  On curve points lhs == rhs iff [8S]B + [8k](-A) - 8R is the neutral element; that is ONE accumulator here: the windows of [8k](-A) over a
// table of the lane's own (d (-A), d = 1 .. 2^WIN - 1, word j of entry e at tab[(e * ED_CW + j) * STRIDE]), then [8S]B from the comb table, then -8R.
// No inversion, no second encoding.
// A lane whose R or A decodes OFF the curve returns false WITHOUT running the reference's arithmetic: there the reference runs its affine formulas on a
// non-point and the outcome hangs on its LSB-first chain (false but for an accident of probability 2^-250).  This is the one decision of this file that is
// not derived from the reference's arithmetic.
template <int STRIDE = 1> ZKT_HD bool ed25519_verify_one(const uint8_t* msg, uint64_t len, const uint8_t* sig, const uint8_t* pub, const uint32_t* btab, uint32_t* tab) {
  uint32_t Rw[8], S[8], Aw[8];
  ld_le_words(sig, Rw, 8); ld_le_words(sig + 32, S, 8); ld_le_words(pub, Aw, 8);
  if (!sc_below_l(S)) return false;                                       // a 256-bit comparison: S + l is rejected
  Fe xr, yr, xa, ya;
  if (!ed25519_decode_one(Rw, xr, yr)) return false;
  uint32_t k8[8], s8[8];
  {                                                                        // the hash comes before the key is decoded: fewer values are alive across it
    uint32_t Rc[8], dw[16], k[8]; uint64_t ra[8], h[8];
    ed25519_encode_affine(xr, yr, Rc);
    sha_words_of_le(Rc, ra); sha_words_of_le(Aw, ra + 4);
    sha512_words<8>(ra, msg, len, h);
    le_words_of_state(h, dw);
    sc_reduce512(dw, k);
    sc_mul8(k, k8);                                                        // (8k) mod l = 8 (k mod l) mod l
    sc_mul8(S, s8);
  }
  if (!ed25519_decode_one(Aw, xa, ya)) return false;
  {
    const Ge a1 = ge_from_affine(fe_neg(xa), ya);                          // -A
    const GeCached c1 = ge_to_cached(a1);
    ge_st_cached<STRIDE>(tab, c1);
    Ge m = a1;
#pragma unroll 1
    for (int d = 2; d <= ED_TAB; ++d) { m = ge_add(m, c1); ge_st_cached<STRIDE>(tab + (size_t)(d - 1) * ED_CW * STRIDE, ge_to_cached(m)); }
  }
  Ge acc = ge_neutral();
  constexpr int NWIN = (253 + ED_WIN - 1) / ED_WIN;                        // 8k mod l < 2^253
#pragma unroll 1
  for (int win = NWIN - 1; win >= 0; --win) {
    const int bit = win * ED_WIN;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { lo = (j == (bit >> 5)) ? k8[j] : lo; hi = (j == (bit >> 5) + 1) ? k8[j] : hi; }
    const uint32_t d = (uint32_t)(((((uint64_t)hi << 32) | lo) >> (bit & 31)) & (uint64_t)ED_TAB);
    if (win != NWIN - 1) {
#pragma unroll 1
      for (int b = 0; b < ED_WIN - 1; ++b) acc = ge_dbl<false>(acc);
      acc = ge_dbl<true>(acc);
    }
    if (d) acc = ge_add(acc, ge_ld_cached<STRIDE>(tab + (size_t)(d - 1) * ED_CW * STRIDE));
  }
  acc = ed25519_add_base_multiple(acc, btab, s8);
  Ge r8 = ge_from_affine(fe_neg(xr), yr);                                  // -R, then three doublings: a torsion part of R dies here
  r8 = ge_dbl<false>(r8); r8 = ge_dbl<false>(r8); r8 = ge_dbl<true>(r8);
  acc = ge_add(acc, ge_to_cached(r8));
  return ge_is_neutral(acc);
}

}  // namespace zkt
