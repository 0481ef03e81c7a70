// TEST-ONLY, part of csrc/hostcheck.cpp (and of tests/c/acc_pairs_check.cpp): host entry points for fp_mul_pair, fp_sqr_pair (fp.h) and for
// xyzz_add_aff_paired (curve.h).  tests/test_acc_pairs_hostcheck.py checks them against python integers.  It DEFINES the two extern "C" functions, so it is included
// by exactly one file of a program: hostcheck.cpp in the host-check libraries, the stand-alone program in its own build, which thereby skips the pairing code.
#pragma once
#include "abi.h"
#include "fq_program.h"
namespace zkt_hostcheck_acc_pairs {           // a scope of its own for the using-directive; the extern "C" names below are global C symbols all the same
using namespace zkt;
// the Montgomery residue of x as canonical + j p, j <= 3: every lazily reduced form a kernel value can take (limbs < 2^28, value < 4p)
Fq fq_lift_canon(const Fq& x, int j) {
  uint32_t w[FqC::ABI_N]; fp_to_words(x, w);
  Fq c = fp_from_words<FqC>(w), s, r; uint32_t bw = 0, carry = 0;        // c < 1.01p: one conditional subtraction
  for (int i = 0; i < FqC::N; ++i) { uint32_t t = c.v[i] - FqC::mod(i) - bw; bw = t >> 31; s.v[i] = t & 0x0fffffffu; }
  if (!bw) c = s;
  for (int i = 0; i < FqC::N; ++i) { uint32_t t = c.v[i] + FqC::kp(j, i) + carry; r.v[i] = t & 0x0fffffffu; carry = t >> 28; }
  return r;
}
extern "C" {
// op 0: fp_mul_pair_impl -> (a b, c d), the interleaved scans themselves; 1: fp_sqr_pair_impl -> (a^2, c^2); 2, 3: fp_mul_pair / fp_sqr_pair, what a caller outside the G1 MSM
// object gets.  The operands enter as canonical + j p, j = two bits of `lifts` each (a, b, c, d from the low end).  Writes the canonical results; returns the number of results
// that break the lazy-limb invariant (0 expected).
int zkt_hostcheck_fq_pair(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, unsigned lifts, uint32_t* o0, uint32_t* o1) {
  const Fq x = fq_lift_canon(ld_fp<FqC>(a), lifts & 3), y = fq_lift_canon(ld_fp<FqC>(b), (lifts >> 2) & 3);
  const Fq z = fq_lift_canon(ld_fp<FqC>(c), (lifts >> 4) & 3), t = fq_lift_canon(ld_fp<FqC>(d), (lifts >> 6) & 3);
  Fq r0, r1;
  switch (op) { case 0: fp_mul_pair_impl(x, y, z, t, r0, r1); break; case 1: fp_sqr_pair_impl(x, z, r0, r1); break; case 2: fp_mul_pair(x, y, z, t, r0, r1); break; default: fp_sqr_pair(x, z, r0, r1); }
  st_fp<FqC>(o0, r0); st_fp<FqC>(o1, r1);
  return (fq_lazy_ok(r0) ? 0 : 1) + (fq_lazy_ok(r1) ? 0 : 1);
}
// The first steps of a G1 bucket through the paired mixed addition.  p, q: affine ABI points (not infinity; they need not lie on the curve), signs bit 0 / bit 1: the entry of
// p / q is negated (the y coordinate, before the addition, as k_accumulate does).
// mode 1: the accumulator holds +-p with ZZ = lambda^2, ZZZ = lambda^3 (lambda: one Fq, must not be zero) and +-q is added by xyzz_add_aff_paired.
// mode 2: the same from an empty accumulator: inf + (+-p), then + (+-q).
// Writes the affine result.
int zkt_hostcheck_g1_acc(int mode, const uint32_t* p, const uint32_t* q, int signs, const uint32_t* lambda, uint32_t* o) {
  typedef FqOps F;
  Aff<F> a = PtIO<F>::ld(p), b = PtIO<F>::ld(q);
  if (a.inf || b.inf || (mode != 1 && mode != 2)) return -1;
  if (signs & 1) a.y = F::neg(a.y);
  if (signs & 2) b.y = F::neg(b.y);
  Xyzz<F> z;
  if (mode == 1) {
    const Fq l = ld_fp<FqC>(lambda), l2 = fp_sqr(l), l3 = fp_mul(l2, l);
    z = xyzz_add_aff_paired<F>(Xyzz<F>{fp_mul(a.x, l2), fp_mul(a.y, l3), l2, l3}, b.x, b.y);
  } else z = xyzz_add_aff_paired<F>(xyzz_add_aff_paired<F>(xyzz_inf<F>(), a.x, a.y), b.x, b.y);
  PtIO<F>::st(o, xyzz_to_aff(z));
  return 0;
}
}  // extern "C"
}  // namespace zkt_hostcheck_acc_pairs
