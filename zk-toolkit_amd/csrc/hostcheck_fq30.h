// TEST-ONLY, part of csrc/hostcheck.cpp: host entry points for the 13 x 30-bit-limb layout of Fq (fp.h, W = 30; Fq30C) that the G1 MSM object runs on.
// Operands and results cross as RAW limbs (13 words, Montgomery form, any lazily reduced value) unless said otherwise, so that tests/test_fq30_hostcheck.py chooses the
// limb patterns itself and checks limbs, size and residue of what comes back against python integers.  It DEFINES extern "C" functions: one includer per program.
#pragma once
#include "abi.h"
namespace zkt_hostcheck_fq30 {
using namespace zkt;
typedef Fq30C C30;
inline Fq30 ld30(const uint32_t* p) { return ld_raw<C30>(p); }
// the device's paired mixed addition: mul_pair / sqr_pair are the interleaved scans themselves (what -DZKT_PAIR_MUL selects in the G1 MSM object)
// (the scans are real functions here: inlined into their callers they make single host functions of tens of thousands of instructions, which take the host
// compiler many minutes)
#define ZKT_HC_FN __attribute__((noinline)) static
ZKT_HC_FN Fq30 hc_mul(const Fq30& a, const Fq30& b) { return fp_mul_impl(a, b); }
ZKT_HC_FN Fq30 hc_sqr(const Fq30& a) { return fp_sqr_impl(a); }
ZKT_HC_FN Fq30 hc_mulsub(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d) { return fp_mul2_impl<C30, true>(a, b, c, d); }
ZKT_HC_FN Fq30 hc_muladd(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d) { return fp_mul2_impl<C30, false>(a, b, c, d); }
ZKT_HC_FN void hc_mul_pair(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d, Fq30& ab, Fq30& cd) { fp_mul_pair_impl(a, b, c, d, ab, cd); }
ZKT_HC_FN void hc_sqr_pair(const Fq30& a, const Fq30& c, Fq30& aa, Fq30& cc) { fp_sqr_pair_impl(a, c, aa, cc); }
struct Fq30PairOps : PrimeOps<C30> {
  static void mul_pair(const E& a, const E& b, const E& c, const E& d, E& ab, E& cd) { hc_mul_pair(a, b, c, d, ab, cd); }
  static void sqr_pair(const E& a, const E& c, E& aa, E& cc) { hc_sqr_pair(a, c, aa, cc); }
};
template <class F> inline bool same_xyzz(const Xyzz<F>& a, const Xyzz<PrimeOps<C30>>& b) {
  bool s = true;
  for (int i = 0; i < C30::N; ++i) s = s && a.X.v[i] == b.X.v[i] && a.Y.v[i] == b.Y.v[i] && a.ZZ.v[i] == b.ZZ.v[i] && a.ZZZ.v[i] == b.ZZZ.v[i];
  return s;
}
extern "C" {
// op 0 fp_mul_impl(a, b) -> o0;  1 fp_sqr_impl(a) -> o0;  2 a b - c d (fp_mul2_impl<true>) -> o0;  3 a b + c d -> o0;
//    4 fp_mul_pair_impl -> (a b, c d);  5 fp_sqr_pair_impl -> (a^2, c^2);  6 fp_mul_pair;  7 fp_sqr_pair (two single calls on the host)
int zkt_hostcheck_fq30_prod(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* o0, uint32_t* o1) {
  const Fq30 x = ld30(a), y = ld30(b), z = ld30(c), t = ld30(d);
  Fq30 r0 = fp_zero<C30>(), r1 = fp_zero<C30>();
  switch (op) {
    case 0: r0 = hc_mul(x, y); break; case 1: r0 = hc_sqr(x); break;
    case 2: r0 = hc_mulsub(x, y, z, t); break; case 3: r0 = hc_muladd(x, y, z, t); break;
    case 4: hc_mul_pair(x, y, z, t, r0, r1); break; case 5: hc_sqr_pair(x, z, r0, r1); break;
    case 6: fp_mul_pair(x, y, z, t, r0, r1); break; case 7: fp_sqr_pair(x, z, r0, r1); break; default: return -1;
  }
  st_raw<C30>(o0, r0); st_raw<C30>(o1, r1);
  return 0;
}
// op 0 add, 1 sub, 2 neg, 3 sub2 (a - b - 2c), 4 fp_is_zero (returned), 5 fp_eq(a, b) (returned).  The limb watch (zkt_hostcheck_fq30_watch) covers the call.
int zkt_hostcheck_fq30_lin(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o) {
  const Fq30 x = ld30(a), y = ld30(b), z = ld30(c);
  Fq30 r = fp_zero<C30>();
  switch (op) {
    case 0: r = fp_add(x, y); break; case 1: r = fp_sub(x, y); break; case 2: r = fp_neg(x); break; case 3: r = fp_sub2(x, y, z); break;
    case 4: return fp_is_zero(x) ? 1 : 0; case 5: return fp_eq(x, y) ? 1 : 0; default: return -1;
  }
  st_raw<C30>(o, r);
  return 0;
}
// the reduction passes on raw limb vectors: form 0 fp_lazy_reduce(v), form 1 fp_lazy_reduce2(v, s)
int zkt_hostcheck_fq30_reduce(int form, const uint32_t* v, const uint32_t* s, uint32_t* o) {
  st_raw<C30>(o, form == 0 ? fp_lazy_reduce<C30>(v) : fp_lazy_reduce2<C30>(v, s));
  return 0;
}
// The extremes the limb intermediates of the sum and difference passes took since the last reset: channel 0 the u32 addend of fp_lazy_reduce (v[i] + carry, taken in
// 64 bits), 1 the 64-bit sum t of either pass, 2 a limb of a difference form before the pass (a + subk - b; subk3 - b - 2c), 3 the carry.  what 0: maximum, 1: minimum.
long long zkt_hostcheck_fq30_watch(int channel, int what) { return what ? limb_watch().lo[channel & 3] : limb_watch().hi[channel & 3]; }
void zkt_hostcheck_fq30_watch_reset() { limb_watch() = LimbWatch(); }
// op 0: 12 canonical words -> raw limbs (fp_from_words);  1: raw limbs -> 12 canonical words (fp_to_words);  2: raw -> raw inverse (fp_inv: out through the words and back)
int zkt_hostcheck_fq30_words(int op, const uint32_t* in, uint32_t* o) {
  if (op == 0) st_raw<C30>(o, fp_from_words<C30>(in));
  else if (op == 1) fp_to_words(ld30(in), o);
  else if (op == 2) st_raw<C30>(o, fp_inv(ld30(in)));
  else return -1;
  return 0;
}
// zkt_hostcheck_g1_acc (hostcheck_acc_pairs.h) in the 30-bit layout.  The sum is formed three ways: xyzz_add_aff (the unpaired sequence), xyzz_add_aff_paired with the
// pairs as two calls, and xyzz_add_aff_paired with the pairs as the interleaved scans (the device's).  Writes the affine result of the last; returns 0 when all three
// accumulators are bit-equal in every limb, 1 otherwise.
int zkt_hostcheck_fq30_g1_acc(int mode, const uint32_t* p, const uint32_t* q, int signs, const uint32_t* lambda, uint32_t* o) {
  typedef PrimeOps<C30> F; typedef Fq30PairOps FP;
  Aff<F> a = PtIO<F>::ld(p), b = PtIO<F>::ld(q);
  if (a.inf || b.inf || (mode != 1 && mode != 2)) return -1;
  if (signs & 1) a.y = F::neg(a.y);
  if (signs & 2) b.y = F::neg(b.y);
  Xyzz<F> z0, z1; Xyzz<FP> z2;
  if (mode == 1) {
    const Fq30 l = ld_fp<C30>(lambda), l2 = fp_sqr(l), l3 = fp_mul(l2, l);
    const Fq30 X = fp_mul(a.x, l2), Y = fp_mul(a.y, l3);
    z0 = xyzz_add_aff<F>(Xyzz<F>{X, Y, l2, l3}, b.x, b.y);
    z1 = xyzz_add_aff_paired<F>(Xyzz<F>{X, Y, l2, l3}, b.x, b.y);
    z2 = xyzz_add_aff_paired<FP>(Xyzz<FP>{X, Y, l2, l3}, b.x, b.y);
  } else {
    z0 = xyzz_add_aff<F>(xyzz_add_aff<F>(xyzz_inf<F>(), a.x, a.y), b.x, b.y);
    z1 = xyzz_add_aff_paired<F>(xyzz_add_aff_paired<F>(xyzz_inf<F>(), a.x, a.y), b.x, b.y);
    z2 = xyzz_add_aff_paired<FP>(xyzz_add_aff_paired<FP>(xyzz_inf<FP>(), a.x, a.y), b.x, b.y);
  }
  PtIO<F>::st(o, xyzz_to_aff(Xyzz<F>{z2.X, z2.Y, z2.ZZ, z2.ZZZ}));
  return same_xyzz(z1, z0) && same_xyzz(z2, z0) ? 0 : 1;
}
}  // extern "C"
}  // namespace zkt_hostcheck_fq30
