// secp256k1 ECDSA, one signature per caller (per lane on the device), as inline host/device math over curve.h and fp.h.
//   Signature            src/building_block/curves/secp256k1/ecdsa.rs:16-20
//   Ecdsa::gen_pub_key   ecdsa.rs:33-35
//   Ecdsa::sign          ecdsa.rs:37-85   (the nonce k is an argument here: the reference draws it at :51)
//   Ecdsa::verify        ecdsa.rs:88-135
// Integers are eight little-endian 32-bit words.  `gtab` is the generator's comb table of zkt_group.hip (k_generator_table<SpOps>):
// entry [w * 15 + d - 1] = d * 16^w * G as raw Montgomery (x, y), w < 64, d = 1..15.
#pragma once
#include "abi.h"
#include "sha256.h"

namespace zkt {

#if !defined(ZKT_ECDSA_WIN)
#define ZKT_ECDSA_WIN 4                 // window width of the u2 * Q chain (profiles/ecdsa_timing.md)
#endif
static constexpr int ECDSA_WIN = ZKT_ECDSA_WIN;
static constexpr int ECDSA_TAB = (1 << ECDSA_WIN) - 1;          // d * Q for d = 1 .. 2^WIN - 1, Jacobian
static constexpr int ECDSA_JW = 3 * SpC::N;                      // words of one Jacobian entry

// z = the digest as a big-endian integer (ecdsa.rs:55, :116): state word h[0] holds the top 32 bits
ZKT_HD void ecdsa_z_from_state(const uint32_t h[8], uint32_t z[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = h[7 - i];
}
ZKT_HD void ecdsa_z_from_digest(const uint8_t* d, uint32_t z[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { const uint8_t* p = d + 4 * (7 - i); z[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
}
// a < m for 8-word integers
template <class C> ZKT_HD bool words_below_modulus(const uint32_t* a) {
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) (void)subb(a[i], C::mod32(i), bw);
  return bw != 0;
}
ZKT_HD bool words_are_zero(const uint32_t* a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a[i];
  return o == 0;
}

// k * G from the comb table: at most 64 mixed additions into `acc`, no doubling.  Every addition is the complete one of curve.h: the running sum can
// equal an entry (k = 2 * 16^w), be its opposite, or be the point at infinity, for chosen scalars.
ZKT_HD Jac<SpOps> ecdsa_add_generator_multiple(Jac<SpOps> acc, const uint32_t* gtab, const uint32_t k[8]) {
#pragma unroll 1
  for (int w = 0; w < 64; ++w) {
    uint32_t kw = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) kw = (j == (w >> 3)) ? k[j] : kw;   // no dynamically indexed register array
    const uint32_t d = (kw >> ((w & 7) * 4)) & 15u;
    if (d) {
      const uint32_t* e = gtab + ((size_t)w * 15 + d - 1) * 2 * SpC::N;
      Aff<SpOps> q; q.x = ld_raw<SpC>(e); q.y = ld_raw<SpC>(e + SpC::N); q.inf = false;
      acc = jac_add_aff(acc, q);
    }
  }
  return acc;
}

// one Jacobian table entry, its 24 words STRIDE words apart: STRIDE = 1 is a contiguous entry (the lane's frame); STRIDE = 64 interleaves the 64 lanes of a
// block word by word (LDS: lane l owns words l, l + 64, ..., so the lanes of a wave fall on 64 different banks whatever entry each reads)
template <int STRIDE> ZKT_HD void ecdsa_st_jac(uint32_t* p, const Jac<SpOps>& a) {
#pragma unroll
  for (int i = 0; i < SpC::N; ++i) { p[i * STRIDE] = a.X.v[i]; p[(SpC::N + i) * STRIDE] = a.Y.v[i]; p[(2 * SpC::N + i) * STRIDE] = a.Z.v[i]; }
}
template <int STRIDE> ZKT_HD Jac<SpOps> ecdsa_ld_jac(const uint32_t* p) {
  Jac<SpOps> a;
#pragma unroll
  for (int i = 0; i < SpC::N; ++i) { a.X.v[i] = p[i * STRIDE]; a.Y.v[i] = p[(SpC::N + i) * STRIDE]; a.Z.v[i] = p[(2 * SpC::N + i) * STRIDE]; }
  return a;
}

// Ecdsa::verify (ecdsa.rs:88-135) for one signature.  z: the digest as an integer, ANY 256-bit value (reduced mod n as f_n.elem does, :117);
// r, s: the signature's integers AS GIVEN, not reduced (:105-112 compares them with n); pk: the public key in the ABI layout, loaded exactly as
// zkt_secp_is_on_curve_batch loads it.  tab: the caller's own memory for the multiples of the public key, ECDSA_TAB entries of ECDSA_JW words, word j of entry e at
// tab[(e * ECDSA_JW + j) * STRIDE] (the lane's frame with STRIDE = 1; the A/B build of profiles/ecdsa_timing.md puts it in LDS with STRIDE = 64).
template <int STRIDE = 1> ZKT_HD bool ecdsa_verify_one(const uint32_t z[8], const uint32_t r[8], const uint32_t s[8], const uint32_t* pk, const uint32_t* gtab, uint32_t* tab) {
  // :105-112 — r, s in [1, n-1]
  if (words_are_zero(r) || words_are_zero(s) || !words_below_modulus<SnC>(r) || !words_below_modulus<SnC>(s)) return false;
  // :94-99 — the public key is a point of the curve, not the point at infinity
  const Aff<SpOps> Q = PtIO<SpOps>::ld(pk);
  if (Q.inf) return false;
  {
    uint32_t w7[8] = {7, 0, 0, 0, 0, 0, 0, 0};
    if (!SpOps::eq(SpOps::sqr(Q.y), SpOps::add(SpOps::mul(SpOps::sqr(Q.x), Q.x), fp_from_words<SpC>(w7)))) return false;
  }
  // :102 — n * pub_key == infinity is NOT evaluated: secp256k1 has cofactor 1, its group of rational points has prime order n, so every point that
  // passed the curve test above is annihilated by n.  (The reference spends a 256-step scalar multiplication on a test that cannot fail.)
  // :116-120 — w = s^-1, u1 = z w, u2 = r w  (mod n)
  const SnE wi = fp_inv(fp_from_words<SnC>(s));
  uint32_t u1[8], u2[8];
  fp_to_words(fp_mul(fp_from_words<SnC>(z), wi), u1);
  fp_to_words(fp_mul(fp_from_words<SnC>(r), wi), u2);
  // :124-126 — u2 * Q by fixed windows over the table d * Q (d = 1 .. 2^WIN - 1), then u1 * G added into the SAME accumulator from the comb table
  {
    Jac<SpOps> q1 = jac_from_aff(Q), m = q1;
    ecdsa_st_jac<STRIDE>(tab, m);
#pragma unroll 1
    for (int d = 2; d <= ECDSA_TAB; ++d) { m = jac_add(m, q1); ecdsa_st_jac<STRIDE>(tab + (size_t)(d - 1) * ECDSA_JW * STRIDE, m); }      // 2Q is the doubling branch of jac_add
  }
  Jac<SpOps> acc = jac_inf<SpOps>();
  constexpr int NWIN = (256 + ECDSA_WIN - 1) / ECDSA_WIN;
#pragma unroll 1
  for (int win = NWIN - 1; win >= 0; --win) {
    const int bit = win * ECDSA_WIN;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { lo = (j == (bit >> 5)) ? u2[j] : lo; hi = (j == (bit >> 5) + 1) ? u2[j] : hi; }
    const uint32_t d = (uint32_t)(((((uint64_t)hi << 32) | lo) >> (bit & 31)) & (uint64_t)ECDSA_TAB);
    if (win != NWIN - 1) {
#pragma unroll 1
      for (int b = 0; b < ECDSA_WIN; ++b) acc = jac_dbl(acc);
    }
    if (d) acc = jac_add(acc, ecdsa_ld_jac<STRIDE>(tab + (size_t)(d - 1) * ECDSA_JW * STRIDE));
  }
  acc = ecdsa_add_generator_multiple(acc, gtab, u1);
  // :128-133 — reject the point at infinity; accept iff r == x mod n.  x = X / Z^2 lies in [0, p) and p > n, so x is r or r + n (the latter only
  // when r + n < p): both candidates are compared projectively, X == c * Z^2, and no inversion is needed.
  if (jac_is_inf(acc)) return false;
  const SpE zz = SpOps::sqr(acc.Z);
  if (SpOps::eq(acc.X, SpOps::mul(fp_from_words<SpC>(r), zz))) return true;
  uint32_t rn[8], c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) rn[i] = addc(r[i], SnC::mod32(i), c);
  if (c != 0 || !words_below_modulus<SpC>(rn)) return false;
  return SpOps::eq(acc.X, SpOps::mul(fp_from_words<SpC>(rn), zz));
}

// Ecdsa::sign (ecdsa.rs:49-84) for one (digest, private key, nonce).  d, k: any 256-bit integers, reduced mod n on load as PrimeFieldElem::new does.
// Returns true where the reference's loop would `continue` and draw another k (k = 0 mod n: kG at infinity :61; r == 0 :67; s == 0 :77); r, s are then zero.
ZKT_HD bool ecdsa_sign_one(const uint32_t z[8], const uint32_t d[8], const uint32_t k[8], const uint32_t* gtab, uint32_t r[8], uint32_t s[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { r[i] = 0; s[i] = 0; }
  const SnE km = fp_from_words<SnC>(k);
  uint32_t kc[8];
  fp_to_words(km, kc);                                                   // k mod n: the comb reads canonical digits
  if (words_are_zero(kc)) return true;                                   // :61
  const Aff<SpOps> P = jac_to_aff(ecdsa_add_generator_multiple(jac_inf<SpOps>(), gtab, kc));      // :58
  if (P.inf) return true;
  uint32_t x[8];
  fp_to_words(P.x, x);
  const SnE rm = fp_from_words<SnC>(x);                                  // :64 — x < p < 2n: the load's conditional subtraction is x mod n
  if (fp_is_zero(rm)) return true;                                       // :67
  const SnE sm = fp_mul(fp_inv(km), fp_add(fp_mul(fp_from_words<SnC>(d), rm), fp_from_words<SnC>(z)));      // :71-74
  if (fp_is_zero(sm)) return true;                                       // :77
  fp_to_words(rm, r); fp_to_words(sm, s);
  return false;
}

}  // namespace zkt
