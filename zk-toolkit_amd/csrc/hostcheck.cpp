// TEST-ONLY: the kernel math headers (fp.h … pairing.h) compiled for the HOST, so the
// `-m "not gpu"` suite can check the exact functions the HIP kernels inline against the
// oracle without a GPU.  Not part of the product: libzkt_hip.so neither links nor calls
// this, and the C ABI in include/zkt.h has no CPU path.  Built by __graft_entry__.build()
// as zk-toolkit_amd/libzkt_hostcheck.so (hipcc --cuda-host-only).
#define ZKT_HOSTCHECK_LIMB_WATCH      // fp.h: record the extremes of the lazy passes' limb intermediates (zkt_hostcheck_fq30_watch)
#include "abi.h"
#include <vector>
#include "fq_program.h"
using namespace zkt;

extern "C" {
unsigned long zkt_hostcheck_bgcd_fallbacks() { return bgcd_fallbacks(); }      // 0 expected: the word-step GCD always ends with b = 1
int zkt_hostcheck_fq_program(uint64_t seed, int steps, const uint32_t* in4, uint32_t* out4) { return fq_program(seed, steps, in4, out4); }
// op: 0 add 1 sub 2 mul 3 sqr 4 neg 5 inv (fp_inv: the word-step binary GCD) 6 inv as x^(p-2) through fp_pow 7 cube 8 pow (b = exponent, ABI_N words per element)
//     9 the classic bit-step binary Euclid on canonical words (bgcd_inverse_classic), 10 the word-step GCD on canonical words (bgcd_inverse)
int zkt_hostcheck_fp(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  auto run = [&](auto tag) {
    typedef decltype(tag) C;
    for (size_t i = 0; i < n; ++i) {
      if (op == 9 || op == 10) { uint32_t w[C::ABI_N]; for (int j = 0; j < C::ABI_N; ++j) w[j] = a[i * C::ABI_N + j]; if (op == 9) bgcd_inverse_classic<C>(w); else bgcd_inverse<C>(w); for (int j = 0; j < C::ABI_N; ++j) o[i * C::ABI_N + j] = w[j]; continue; }
      Fp<C> x = ld_fp<C>(a + i * C::ABI_N), y = b ? ld_fp<C>(b + i * C::ABI_N) : fp_zero<C>(), r;
      switch (op) {
        case 0: r = fp_add(x, y); break; case 1: r = fp_sub(x, y); break; case 2: r = fp_mul(x, y); break;
        case 3: r = fp_sqr(x); break; case 4: r = fp_neg(x); break; case 6: { uint32_t e[C::ABI_N]; for (int j = 0; j < C::ABI_N; ++j) e[j] = C::pm2(j); r = fp_pow(x, e, C::ABI_N); } break;
        case 7: r = fp_mul(fp_sqr(x), x); break; case 8: r = fp_pow(x, b + i * C::ABI_N, C::ABI_N); break; default: r = fp_inv(x);
      }
      st_fp<C>(o + i * C::ABI_N, r);
    }
  };
  switch (field) { case 0: run(FqC{}); break; case 1: run(FrC{}); break; case 2: run(SpC{}); break; default: run(SnC{}); }
  return 0;
}
// Both Fq2 products (four-scan lazy form and three-scan Karatsuba form, tower.h / fp.h) on non-canonical representatives: every operand
// coordinate is moved to canonical + j*p (j < 3, selected by two bits of `lifts` each).  Writes the canonical product; returns the number
// of disagreements between the two forms or with the lazy-limb invariants (0 expected).
int zkt_hostcheck_fq2_mul_lifted(const uint32_t* a, const uint32_t* b, unsigned lifts, uint32_t* o) {
  Fq2 x = ld_fq2(a), y = ld_fq2(b);
  x.c0 = fq_lift(x.c0, (lifts & 3) % 3); x.c1 = fq_lift(x.c1, ((lifts >> 2) & 3) % 3);
  y.c0 = fq_lift(y.c0, ((lifts >> 4) & 3) % 3); y.c1 = fq_lift(y.c1, ((lifts >> 6) & 3) % 3);
  const Fq2 four{fp_mulsub(x.c0, y.c0, x.c1, y.c1), fp_muladd(x.c0, y.c1, x.c1, y.c0)};
  Fq2 three; fp2_mul_kara(x.c0, x.c1, y.c0, y.c1, three.c0, three.c1);
  int bad = 0;
  if (!fq_lazy_ok(three.c0) || !fq_lazy_ok(three.c1)) ++bad;
  if (!fp_eq(four.c0, three.c0) || !fp_eq(four.c1, three.c1)) ++bad;
  st_fq2(o, three);
  return bad;
}
// op: 0 add 1 sub 2 mul 3 inv 4 neg 5 mul_xi/mul_v 6 sqr 7 frob1 8 frob2 9 conj
int zkt_hostcheck_tower(int deg, int op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  if (deg == 2) {
    Fq2 x = ld_fq2(a), y = b ? ld_fq2(b) : fq2_zero(), r;
    switch (op) { case 0: r = fq2_add(x, y); break; case 1: r = fq2_sub(x, y); break; case 2: r = fq2_mul(x, y); break;
      case 3: r = fq2_inv(x); break; case 4: r = fq2_neg(x); break; case 5: r = fq2_mul_xi(x); break; default: r = fq2_sqr(x); }
    st_fq2(o, r);
  } else if (deg == 6) {
    Fq6 x = ld_fq6(a), y = b ? ld_fq6(b) : fq6_zero(), r;
    switch (op) { case 0: r = fq6_add(x, y); break; case 1: r = fq6_sub(x, y); break; case 2: r = fq6_mul(x, y); break;
      case 3: r = fq6_inv(x); break; case 4: r = fq6_neg(x); break; default: r = fq6_mul_v(x); }
    st_fq6(o, r);
  } else {
    Fq12 x = ld_fq12(a), y = b ? ld_fq12(b) : fq12_one(), r;
    switch (op) { case 0: r = fq12_add(x, y); break; case 1: r = fq12_sub(x, y); break; case 2: r = fq12_mul(x, y); break;
      case 3: r = fq12_inv(x); break; case 4: r = fq12_neg(x); break; case 6: r = fq12_sqr(x); break;
      case 7: r = fq12_frob<1>(x); break; case 8: r = fq12_frob<2>(x); break; case 10: r = fq12_cyclotomic_sqr(x); break; default: r = fq12_conj(x); }
    st_fq12(o, r);
  }
  return 0;
}
}  // extern "C"
template <class F> static void pt_add(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  Aff<F> p = PtIO<F>::ld(a), q = PtIO<F>::ld(b);
  PtIO<F>::st(o, jac_to_aff(jac_add_aff(jac_from_aff(p), q)));
}
template <class F> static void pt_add_full(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  // exercise jac_add and the XYZZ formulas too: ((2a) + b) - a computed two ways must agree with a + b
  Aff<F> p = PtIO<F>::ld(a), q = PtIO<F>::ld(b);
  Jac<F> j = jac_add(jac_dbl(jac_from_aff(p)), jac_from_aff(q));
  Aff<F> np = p; if (!np.inf) np.y = F::neg(np.y);
  j = jac_add_aff(j, np);
  Xyzz<F> z = xyzz_inf<F>();
  if (!p.inf) z = xyzz_add_aff(z, p.x, p.y);
  if (!q.inf) z = xyzz_add_aff(z, q.x, q.y);
  Xyzz<F> z2 = xyzz_add(z, xyzz_inf<F>());
  Aff<F> r1 = jac_to_aff(j), r2 = xyzz_to_aff(z2), r3 = jac_to_aff(xyzz_to_jac(z));
  bool same = (r1.inf == r2.inf) && (r1.inf || (F::eq(r1.x, r2.x) && F::eq(r1.y, r2.y)));
  same = same && (r1.inf == r3.inf) && (r1.inf || (F::eq(r1.x, r3.x) && F::eq(r1.y, r3.y)));
  if (!same) { r1.inf = true; }   // poison: a mismatch between formula sets shows up as a wrong answer
  PtIO<F>::st(o, r1);
}
template <class F> static void pt_mul(const uint32_t* a, const uint32_t* k, int klimbs, uint32_t* o) {
  PtIO<F>::st(o, jac_to_aff(scalar_mul_aff(PtIO<F>::ld(a), k, klimbs)));
}
extern "C" {
// grp: 0 G1, 1 G2, 2 secp256k1.  op: 0 add (mixed), 1 add via the other formula sets, 2 scalar mul (b = scalar, u32 limbs)
int zkt_hostcheck_group(int grp, int op, const uint32_t* a, const uint32_t* b, int klimbs, uint32_t* o) {
  if (grp == 0) { if (op == 0) pt_add<FqOps>(a, b, o); else if (op == 1) pt_add_full<FqOps>(a, b, o); else pt_mul<FqOps>(a, b, klimbs, o); }
  else if (grp == 1) { if (op == 0) pt_add<Fq2Ops>(a, b, o); else if (op == 1) pt_add_full<Fq2Ops>(a, b, o); else pt_mul<Fq2Ops>(a, b, klimbs, o); }
  else { if (op == 0) pt_add<SpOps>(a, b, o); else if (op == 1) pt_add_full<SpOps>(a, b, o); else pt_mul<SpOps>(a, b, klimbs, o); }
  return 0;
}
// which: 0 calc_g1_g2, 1 calc_g2_g1, 2 weil
int zkt_hostcheck_miller_exact(int which, const uint32_t* g1, const uint32_t* g2, uint32_t* o) {
  Aff<FqOps> p = PtIO<FqOps>::ld(g1); Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(g2);
  if (p.inf || q.inf) return 2;
  Fq12 r; bool bad = false;
  if (which == 0) r = miller_g1_g2_exact(p.x, p.y, q.x, q.y, bad);
  else if (which == 1) r = miller_g2_g1_exact(q.x, q.y, p.x, p.y);
  else r = fq12_mul(miller_g1_g2_exact(p.x, p.y, q.x, q.y, bad), fq12_inv(miller_g2_g1_exact(q.x, q.y, p.x, p.y)));
  if (bad) return 2;
  st_fq12(o, r);
  return 0;
}
int zkt_hostcheck_tate(const uint32_t* g1, const uint32_t* g2, uint32_t* o) {
  Aff<FqOps> p = PtIO<FqOps>::ld(g1); Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(g2);
  if (p.inf || q.inf) return 2;
  // the three passes of launch_tate (zkt_tate.hip): 127-step loop for P in G1 and Q in G2, 255-step loop for Q on E' outside G2, the reference's own chain otherwise
  Fq12 f; bool in_g1 = false, bad;
  const int route = tate_short(p.x, p.y, q.x, q.y, f);
  if (route == TATE_ROUTE_SHORT) { st_fq12(o, f); return 0; }
  if (route == TATE_ROUTE_LONG) {
    f = miller_g1_g2(p.x, p.y, q.x, q.y, in_g1);
    if (in_g1) { st_fq12(o, final_exponentiation(f)); return 50; }          // 50: value produced by the 255-step loop
  }
  f = miller_g1_g2_exact(p.x, p.y, q.x, q.y, bad);
  if (bad) return 2;
  if (fq12_is_zero(f)) { for (int k = 0; k < 144; ++k) o[k] = 0; return 100; }
  st_fq12(o, final_exponentiation(f));
  return 100;                             // 100: value produced by the exact path
}
// the membership tests that guard the 127-step loop: bit 0 = P on E, bit 1 = r P == infinity (from the loop), bit 2 = Q in G2, bit 3 = Q on E'
int zkt_hostcheck_short_loop_guards(const uint32_t* g1, const uint32_t* g2) {
  Aff<FqOps> p = PtIO<FqOps>::ld(g1); Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(g2);
  if (p.inf || q.inf) return -1;
  bool ok; (void)miller_g1_g2_short(p.x, p.y, q.x, q.y, ok);
  return (g1_on_curve(p.x, p.y) ? 1 : 0) | (ok ? 2 : 0) | (g2_on_curve(q.x, q.y) && g2_in_subgroup(q.x, q.y) ? 4 : 0) | (g2_on_curve(q.x, q.y) ? 8 : 0);
}
// The 63-step (optimal-ate) product of the deciding entry points (pairing.h): kv pairs whose Q runs its own chain, then kf pairs whose Q comes as a line table built here.
// Returns -1 when a guard refuses an argument (the kernels then leave the element to the older routes), else writes final_exponentiation(prod f_{|x|,Q_k}(P_k)).
// bit 8 of the return value: the table builder's G2 verdict for the tabulated points disagreed with g2_in_subgroup (0 expected).
int zkt_hostcheck_ate_product(int kv, int kf, const uint32_t* g1, const uint32_t* g2, uint32_t* o) {
  const int K = kv + kf;
  if (K < 1 || K > 3) return -2;
  Fq xp[3], yp[3]; Fq2 xq[3], yq[3];
  static uint32_t tabs[3][ATE_LINES * ATE_LINE_WORDS];
  const uint32_t* tp[3] = {tabs[0], tabs[1], tabs[2]};
  int odd = 0;
  for (int k = 0; k < K; ++k) {
    Aff<FqOps> p = PtIO<FqOps>::ld(g1 + k * ABI_G1_WORDS); Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(g2 + k * ABI_G2_WORDS);
    if (p.inf || q.inf) return -3;
    if (!g1_on_curve(p.x, p.y) || !g1_in_subgroup(p.x, p.y) || !g2_on_curve(q.x, q.y)) return -1;
    xp[k] = p.x; yp[k] = p.y; xq[k] = q.x; yq[k] = q.y;
    if (k >= kv) {
      const bool in = ate_line_table(q.x, q.y, tabs[k - kv]);
      if (in != g2_in_subgroup(q.x, q.y)) odd = 256;
      if (!in) return -1 - odd;
    }
  }
  bool q_ok = false; Fq12 f;
  if (kv == 1 && kf == 0) f = miller_ate_multi<1, 0>(xp, yp, xq, yq, tp, q_ok);
  else if (kv == 2 && kf == 0) f = miller_ate_multi<2, 0>(xp, yp, xq, yq, tp, q_ok);
  else if (kv == 3 && kf == 0) f = miller_ate_multi<3, 0>(xp, yp, xq, yq, tp, q_ok);
  else if (kv == 1 && kf == 2) f = miller_ate_multi<1, 2>(xp, yp, xq, yq, tp, q_ok);
  else if (kv == 0 && kf == 1) f = miller_ate_multi<0, 1>(xp, yp, xq, yq, tp, q_ok);
  else return -2;
  if (!q_ok) return -1;
  st_fq12(o, final_exponentiation_3h(f));       // the exponent the deciding kernels use (three times the exact one)
  return odd;
}
}

// ---- whole batches, for the case lists of tests/prim_cases.py (tests/test_prim_cases.py) ------------------------------------------------------------
// The 8-word branch of k_fp_op (zkt_field.hip) REPEATED, not shared: canonical values in and out (fp_canon32, then fp_mul(fp_mul(x, y), R^2); the inverse of x R), where
// zkt_hostcheck_fp goes through ld_fp / st_fp.  tests/test_prim_cases.py compares the two texts between the marker comments after stripping whitespace.
// op: 0 add 1 sub 2 mul 3 sqr 4 neg 5 inv 7 cube (the numbering of zkt_hostcheck_fp).  Returns the lowest index whose inverse was asked of zero, or -1.
template <class C> static long fp_canon_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  enum { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_SQR = 3, OP_NEG = 4, OP_INV = 5, OP_CUBE = 7 };
  long first = -1;
  // `atomicMin`, `err` and `OP` exist under these names ONLY so that the kernel's text below compiles here unchanged (the device has the HIP intrinsic, an error
  // word in memory and a template parameter); the loop body keeps the kernel's indentation for the same reason: the text comparison ignores white space only.
  auto atomicMin = [](long* e, unsigned long long i) { if (*e < 0 || (long)i < *e) *e = (long)i; };
  long* err = &first;
  const int OP = op;
  for (size_t i = 0; i < n; ++i) {
  // canonical 32-bit-limb fields: any 256-bit input is first reduced mod the order, as PrimeFieldElem::new does (prime_field_elem.rs:263-272)
  Fp<C> x = fp_canon32(ld_raw<C>(a + i * C::N)), r, r2;
  for (int j = 0; j < C::N; ++j) r2.v[j] = C::r2(j);
  if (OP == OP_ADD) r = fp_add(x, fp_canon32(ld_raw<C>(b + i * C::N)));          // canonical in, canonical out
  else if (OP == OP_SUB) r = fp_sub(x, fp_canon32(ld_raw<C>(b + i * C::N)));
  else if (OP == OP_NEG) r = fp_neg(x);
  else if (OP == OP_MUL) r = fp_mul(fp_mul(x, fp_canon32(ld_raw<C>(b + i * C::N))), r2);     // (a b R^-1) R^2 R^-1 = a b
  else if (OP == OP_SQR) r = fp_mul(fp_mul(x, x), r2);
  else if (OP == OP_CUBE) { Fp<C> xm = fp_mul(x, r2); r = fp_mul(fp_mul(xm, xm), x); }        // (xR)(xR)/R = x^2 R;  x^2 R * x / R = x^3
  else {                                                             // safe_inv: Err on zero (prime_field_elem.rs:379-382)
    if (fp_is_zero(x)) { atomicMin(err, (unsigned long long)i); r = x; }
    else {
      Fp<C> one = fp_zero<C>(); one.v[0] = 1;
      r = fp_mul(fp_inv(fp_mul(x, r2)), one);
    }
  }
  st_raw<C>(out + i * C::N, r);
  }
  return first;
}
extern "C" {
long zkt_hostcheck_fp_canon(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  switch (field) { case 1: return fp_canon_run<FrC>(op, a, b, o, n); case 2: return fp_canon_run<SpC>(op, a, b, o, n); case 3: return fp_canon_run<SnC>(op, a, b, o, n); }
  return -2;                                                            // Fq is a lazy-limb field: zkt_hostcheck_fp is its kernel's sequence
}
// the kernels' own zero test on the loaded value (k_fp_op, W = 28 branch: fp_is_zero after ld_fp): the lowest index holding zero, or -1
long zkt_hostcheck_fp_first_zero(int field, const uint32_t* a, size_t n) {
  auto run = [&](auto tag) -> long { typedef decltype(tag) C; for (size_t i = 0; i < n; ++i) if (fp_is_zero(ld_fp<C>(a + i * C::ABI_N))) return (long)i; return -1; };
  switch (field) { case 0: return run(FqC{}); case 1: return run(FrC{}); case 2: return run(SpC{}); default: return run(SnC{}); }
}
// the other field kernels of zkt_field.hip on whole batches: op 0 pow (k_fp_pow: e_words 32-bit words per exponent, shared != 0: one exponent for every element),
// 1 scale (k_fp_scale: b = one factor), 2 sum (the fold of fp_add from zero that k_fp_sum's lanes, LDS tree and second launch reassociate; one output element)
int zkt_hostcheck_fp_vec(int field, int op, const uint32_t* a, const uint32_t* b, int e_words, int shared, uint32_t* o, size_t n) {
  auto run = [&](auto tag) {
    typedef decltype(tag) C; constexpr int A = C::ABI_N;
    if (op == 2) { Fp<C> acc = fp_zero<C>(); for (size_t i = 0; i < n; ++i) acc = fp_add(acc, ld_fp<C>(a + i * A)); st_fp<C>(o, acc); return; }
    for (size_t i = 0; i < n; ++i) {
      if (op == 0) st_fp<C>(o + i * A, fp_pow(ld_fp<C>(a + i * A), b + (shared ? 0 : i * (size_t)e_words), e_words));
      else st_fp<C>(o + i * A, fp_mul(ld_fp<C>(a + i * A), ld_fp<C>(b)));
    }
  };
  switch (field) { case 0: run(FqC{}); break; case 1: run(FrC{}); break; case 2: run(SpC{}); break; default: run(SnC{}); }
  return 0;
}
// k_tower_op (zkt_field.hip) on a batch, zero test included: op 0 add 1 sub 2 mul 3 inv 4 neg 5 reduce (mul_xi / mul_v; not for Fq12).
// Returns the lowest index whose inverse was asked of zero, or -1.
long zkt_hostcheck_tower_batch(int deg, int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  long first = -1;
  for (size_t i = 0; i < n; ++i) {
    const size_t w = (size_t)deg * 12 * i;
    bool zero = false;
    if (deg == 2) zero = op == 3 && fq2_is_zero(ld_fq2(a + w));
    else if (deg == 6) zero = op == 3 && fq6_is_zero(ld_fq6(a + w));
    else { const Fq12 x = ld_fq12(a + w); zero = op == 3 && fq6_is_zero(x.c0) && fq6_is_zero(x.c1); }
    if (zero) { if (first < 0) first = (long)i; for (int j = 0; j < deg * 12; ++j) o[w + j] = a[w + j]; continue; }
    if (deg == 12 && op == 5) return -2;
    zkt_hostcheck_tower(deg, op, a + w, b ? b + w : a + w, o + w);
  }
  return first;
}
// k_fq12_pow: every element to one run-time exponent of nl 32-bit words
int zkt_hostcheck_fq12_pow(const uint32_t* a, const uint32_t* e, int nl, uint32_t* o, size_t n) {
  for (size_t i = 0; i < n; ++i) st_fq12(o + i * 144, fq12_pow(ld_fq12(a + i * 144), e, nl));
  return 0;
}
}  // extern "C"
// the curve constants of zkt_group.hip (CurveB lives in that kernel file, so it is repeated here): y^2 = x^3 + 4, x^3 + 4(1+u), x^3 + 7
template <class F> struct HostCurveB;
template <> struct HostCurveB<FqOps> { static Fq b() { uint32_t w[12] = {4}; return fp_from_words<FqC>(w); } };
template <> struct HostCurveB<Fq2Ops> { static Fq2 b() { const Fq f = HostCurveB<FqOps>::b(); return Fq2{f, f}; } };
template <> struct HostCurveB<SpOps> { static SpE b() { uint32_t w[8] = {7}; return fp_from_words<SpC>(w); } };
template <class F> static void pt_batch(int op, const uint32_t* a, const uint32_t* b, int kw, int k_stride, uint32_t* o, size_t n) {
  constexpr int W = PtIO<F>::WORDS;
  for (size_t i = 0; i < n; ++i) {
    Aff<F> p = PtIO<F>::ld(a + i * W);
    if (op == 0) PtIO<F>::st(o + i * W, jac_to_aff(jac_add_aff(jac_from_aff(p), PtIO<F>::ld(b + i * W))));                 // k_group_add
    else if (op == 2) PtIO<F>::st(o + i * W, jac_to_aff(scalar_mul_aff<F>(p, b + i * (size_t)k_stride, kw)));              // k_group_mul, 2..12 words
    else if (op == 3) { if (!p.inf) p.y = F::neg(p.y); PtIO<F>::st(o + i * W, p); }                                        // k_group_neg
    else if (op == 7) o[i] = !p.inf && F::eq(F::sqr(p.y), F::add(F::mul(F::sqr(p.x), p.x), HostCurveB<F>::b()));               // k_group_pred<F, 0>
    else { uint32_t k[SCALAR_MAX_LIMBS]; for (int j = 0; j < kw; ++j) k[j] = b[j]; o[i] = p.inf || jac_is_inf(scalar_mul_aff<F>(p, k, kw)); }   // k_group_pred<F, 1>: b = the order
  }
}
// the sum kernels' shape (k_group_sum_partials / k_group_sum_finish): `lanes` strided mixed-addition accumulators folded pairwise by jac_add from the top half down
template <class F> static void pt_sum(const uint32_t* a, size_t n, int lanes, uint32_t* o) {
  constexpr int W = PtIO<F>::WORDS;
  std::vector<Jac<F>> acc((size_t)lanes, jac_inf<F>());
  for (size_t i = 0; i < n; ++i) acc[i % lanes] = jac_add_aff(acc[i % lanes], PtIO<F>::ld(a + i * W));
  for (int d = lanes / 2; d >= 1; d >>= 1) for (int l = 0; l < d; ++l) acc[l] = jac_add(acc[l], acc[l + d]);
  PtIO<F>::st(o, jac_to_aff(acc[0]));
}
// the generator's comb table and its digit walk (k_generator_table / k_generator_mul, zkt_group.hip): table[w * 15 + d - 1] = d * 16^w * G, a product is at most 64 mixed additions
template <class F> static void pt_comb(const uint32_t* gen_abi, const uint32_t* scalars, uint32_t* o, size_t n) {
  constexpr int W = PtIO<F>::WORDS;
  static std::vector<Aff<F>> table;
  if (table.empty()) for (int t = 0; t < 64 * 15; ++t) {
    const int w = t / 15; const uint32_t d = (uint32_t)(t % 15) + 1u;
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    k[w >> 3] = d << ((w & 7) * 4);
    table.push_back(jac_to_aff(scalar_mul_aff<F>(PtIO<F>::ld(gen_abi), k, 8)));
  }
  for (size_t i = 0; i < n; ++i) {
    Jac<F> acc = jac_inf<F>();
    for (int w = 0; w < 64; ++w) {
      const uint32_t d = (scalars[i * 8 + (w >> 3)] >> ((w & 7) * 4)) & 15u;
      if (d) { Aff<F> q = table[(size_t)w * 15 + d - 1]; q.inf = false; acc = jac_add_aff(acc, q); }
    }
    PtIO<F>::st(o + i * W, jac_to_aff(acc));
  }
}
extern "C" {
// grp: 0 G1, 1 G2, 2 secp256k1.  op: 0 add, 2 scalar mul (b: kw 32-bit words per scalar, k_stride 0 = one scalar for every point), 3 neg, 4 order * P == infinity (b = order, kw words; o: one word per point), 7 on the curve and not at infinity (o: one word per point),
// 5 sum of the n points with `kw` lanes (o: one point), 6 generator products through the comb table (a = the generator, b = n scalars of 8 words; G1 and G2)
int zkt_hostcheck_group_batch(int grp, int op, const uint32_t* a, const uint32_t* b, int kw, int k_stride, uint32_t* o, size_t n) {
  if (op == 5) { if (kw < 1 || (kw & (kw - 1))) return -1; if (grp == 0) pt_sum<FqOps>(a, n, kw, o); else if (grp == 1) pt_sum<Fq2Ops>(a, n, kw, o); else pt_sum<SpOps>(a, n, kw, o); return 0; }
  if (op == 6) { if (grp == 0) pt_comb<FqOps>(a, b, o, n); else if (grp == 1) pt_comb<Fq2Ops>(a, b, o, n); else return -1; return 0; }
  if (kw > SCALAR_MAX_LIMBS) return -1;
  if (grp == 0) pt_batch<FqOps>(op, a, b, kw, k_stride, o, n); else if (grp == 1) pt_batch<Fq2Ops>(op, a, b, kw, k_stride, o, n); else pt_batch<SpOps>(op, a, b, kw, k_stride, o, n);
  return 0;
}
}  // extern "C"

// ---- SHA-256 and secp256k1 ECDSA (sha256.h, ecdsa.h): the per-message and per-signature functions the kernels of zkt_ecdsa.hip run, on the host ----------------
#include "ecdsa.h"
#include "host_abi.h"
namespace {
// the generator's comb table in the layout of k_generator_table<SpOps>: [w * 15 + d - 1] = d * 16^w * G, raw Montgomery (x, y)
const uint32_t* secp_comb_table() {
  static std::vector<uint32_t> t;
  if (!t.empty()) return t.data();
  t.resize((size_t)64 * 15 * 2 * SpC::N);
  Aff<SpOps> base = PtIO<SpOps>::ld((const uint32_t*)&SECP_GEN);
  for (int w = 0; w < 64; ++w) {
    Jac<SpOps> m = jac_from_aff(base);
    for (int d = 1; d <= 15; ++d) {
      const Aff<SpOps> a = jac_to_aff(m);
      uint32_t* e = t.data() + ((size_t)w * 15 + d - 1) * 2 * SpC::N;
      st_raw<SpC>(e, a.x); st_raw<SpC>(e + SpC::N, a.y);
      m = jac_add_aff(m, base);
    }
    base = jac_to_aff(m);                                           // 16 * base
  }
  return t.data();
}
}  // namespace
extern "C" {
// digest (32 bytes) of msg[0..len) by the padding, block loader and compression the kernels use; msg may have any alignment
int zkt_hostcheck_sha256(const uint8_t* msg, size_t len, uint8_t* digest) { uint32_t h[8]; sha256_words(msg, len, h); sha256_store_digest(h, digest); return 0; }
// one compression: h (8 words) updated by the block w (16 big-endian words)
int zkt_hostcheck_sha256_compress(uint32_t* h, const uint32_t* w) { uint32_t blk[16]; for (int i = 0; i < 16; ++i) blk[i] = w[i]; sha256_compress(h, blk); return 0; }
// byte `pos` of the padded message of a len-byte msg (pad_msg), and the padded length through *padded_len
int zkt_hostcheck_sha256_pad(const uint8_t* msg, size_t len, size_t pos, size_t* padded_len) {
  const uint64_t pl = ((len + 8) / 64 + 1) * 64; if (padded_len) *padded_len = (size_t)pl;
  return pos < pl ? (int)sha256_padded_byte(msg, len, pl, pos) : -1;
}
// ecdsa_verify_one: digest 32 bytes, sig = {r, s} 16 words, pk = one ABI point (18 words); returns 1/0
int zkt_hostcheck_ecdsa_verify(const uint8_t* digest, const uint32_t* sig, const uint32_t* pk) {
  uint32_t z[8], tab[ECDSA_TAB * ECDSA_JW];
  ecdsa_z_from_digest(digest, z);
  return ecdsa_verify_one<1>(z, sig, sig + 8, pk, secp_comb_table(), tab) ? 1 : 0;
}
// ecdsa_sign_one: digest 32 bytes, d and k 8 words each; sig = {r, s} 16 words out; returns the retry flag
int zkt_hostcheck_ecdsa_sign(const uint8_t* digest, const uint32_t* d, const uint32_t* k, uint32_t* sig) {
  uint32_t z[8];
  ecdsa_z_from_digest(digest, z);
  return ecdsa_sign_one(z, d, k, secp_comb_table(), sig, sig + 8) ? 1 : 0;
}
}  // extern "C"

// ---- the paired Fq products and the paired mixed addition of the G1 accumulate loop: zkt_hostcheck_fq_pair, zkt_hostcheck_g1_acc.  Kept in a header of their
// own so that the stand-alone sanitizer program (tests/c/acc_pairs_check.cpp) compiles them without the pairing code above.
#include "hostcheck_acc_pairs.h"

// ---- Fq on 13 x 30-bit limbs (fp.h, W = 30: the G1 MSM object's layout): products, sums, reductions, word conversions, inversion and the mixed addition on raw limbs
#include "hostcheck_fq30.h"

// ---- SHA-512 and Ed25519 (sha512.h, fe25519.h, ed25519.h): the per-message, per-key and per-signature functions the kernels of zkt_ed25519.hip run, on the host ----
#include "ed25519.h"
namespace {
// the base point's comb table as k_ed25519_table writes it: [w * 15 + d - 1] = d * 16^w * B as (y-x, y+x, 2dxy)
const uint32_t* ed25519_comb_table() {
  static std::vector<uint32_t> t;
  if (!t.empty()) return t.data();
  t.resize((size_t)ED_COMB_ENTRIES * ED_PRE_WORDS);
  for (int e = 0; e < ED_COMB_ENTRIES; ++e) ed25519_comb_entry(e, t.data() + (size_t)e * ED_PRE_WORDS);
  return t.data();
}
}  // namespace
extern "C" {
// digest (64 bytes) of prefix[0..plen) ‖ msg[0..len), plen in {0, 32, 64}: the prefix goes in as register words, as the kernels pass it; msg may have any alignment
int zkt_hostcheck_sha512(const uint8_t* prefix, size_t plen, const uint8_t* msg, size_t len, uint8_t* digest) {
  uint64_t pre[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h[8];
  if (plen != 0 && plen != 32 && plen != 64) return -1;
  for (size_t i = 0; i < plen; ++i) pre[i / 8] |= (uint64_t)prefix[i] << (56 - 8 * (i % 8));
  if (plen == 0) sha512_words<0>(pre, msg, len, h); else if (plen == 32) sha512_words<4>(pre, msg, len, h); else sha512_words<8>(pre, msg, len, h);
  sha512_store_digest(h, digest);
  return 0;
}
// one compression: h (8 words) updated by the block w (16 big-endian words)
int zkt_hostcheck_sha512_compress(uint64_t* h, const uint64_t* w) { uint64_t blk[16]; for (int i = 0; i < 16; ++i) blk[i] = w[i]; sha512_compress(h, blk); return 0; }
// byte `pos` of the padded message of a len-byte msg (pad_msg), and the padded length through *padded_len
int zkt_hostcheck_sha512_pad(const uint8_t* msg, size_t len, size_t pos, size_t* padded_len) {
  const uint64_t pl = sha512_padded_len(len); if (padded_len) *padded_len = (size_t)pl;
  return pos < pl ? (int)sha512_padded_byte(msg, 0, len, pl, pos) : -1;
}
// field mod 2^255 - 19: a, b are ANY 8-word values (not reduced), o is the canonical result
int zkt_hostcheck_fe25519_mul(const uint32_t* a, const uint32_t* b, uint32_t* o) { fe_to_words(fe_mul(fe_from_words(a), fe_from_words(b)), o); return 0; }
int zkt_hostcheck_fe25519_sqr(const uint32_t* a, uint32_t* o) { fe_to_words(fe_sqr(fe_from_words(a)), o); return 0; }
int zkt_hostcheck_fe25519_inv(const uint32_t* a, uint32_t* o) { fe_to_words(fe_inv(fe_from_words(a)), o); return 0; }
// op 0 add, 1 sub, 2 neg (b unused)
int zkt_hostcheck_fe25519_lin(int op, const uint32_t* a, const uint32_t* b, uint32_t* o) {
  const Fe x = fe_from_words(a), y = fe_from_words(b);
  fe_to_words(op == 0 ? fe_add(x, y) : op == 1 ? fe_sub(x, y) : fe_neg(x), o); return 0;
}
// fe_sqrt_ratio: x = (u/v)^((q+3)/8), times I if its square is not u/v; returns whether the square of the x handed back is u/v (v != 0)
int zkt_hostcheck_fe25519_sqrt_ratio(const uint32_t* u, const uint32_t* v, uint32_t* x) {
  Fe r; const bool ok = fe_sqrt_ratio(fe_from_words(u), fe_from_words(v), r); fe_to_words(r, x); return ok ? 1 : 0;
}
// integers mod l: x (16 words) mod l; (a b + c) mod l
int zkt_hostcheck_sc25519_reduce512(const uint32_t* x, uint32_t* r) { sc_reduce512(x, r); return 0; }
int zkt_hostcheck_sc25519_muladd(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* r) { sc_muladd(a, b, c, r); return 0; }
// ed25519_decode_one: enc 32 bytes -> xy = x (8 words), y (8 words), canonical; returns the on-curve flag
int zkt_hostcheck_ed25519_decode(const uint8_t* enc, uint32_t* xy) {
  uint32_t w[8]; Fe x, y;
  ld_le_words(enc, w, 8);
  const bool on = ed25519_decode_one(w, x, y);
  fe_to_words(x, xy); fe_to_words(y, xy + 8);
  return on ? 1 : 0;
}
// ed25519_pub_from_scalar: the already pruned 32-byte scalar s (so that s >= q can be given) -> enc(B (s mod q))
int zkt_hostcheck_ed25519_pub_from_scalar(const uint8_t* s, uint8_t* pub) {
  uint32_t w[8], enc[8];
  ld_le_words(s, w, 8);
  ed25519_pub_from_scalar(w, ed25519_comb_table(), enc);
  st_le_words(pub, enc, 8);
  return 0;
}
int zkt_hostcheck_ed25519_public_key(const uint8_t* prv, uint8_t* pub) { ed25519_public_key_one(prv, ed25519_comb_table(), pub); return 0; }
int zkt_hostcheck_ed25519_sign(const uint8_t* msg, size_t len, const uint8_t* prv, uint8_t* sig) { ed25519_sign_one(msg, len, prv, ed25519_comb_table(), sig); return 0; }
// ed25519_verify_one with the window table in the caller's frame (stride 1) or word-interleaved as the LDS form lays it out (stride 64)
int zkt_hostcheck_ed25519_verify(const uint8_t* msg, size_t len, const uint8_t* sig, const uint8_t* pub, int stride) {
  if (stride == 64) { std::vector<uint32_t> tab((size_t)ED_TAB * ED_CW * 64); return ed25519_verify_one<64>(msg, len, sig, pub, ed25519_comb_table(), tab.data() + 5) ? 1 : 0; }
  uint32_t tab[ED_TAB * ED_CW];
  return ed25519_verify_one<1>(msg, len, sig, pub, ed25519_comb_table(), tab) ? 1 : 0;
}
}  // extern "C"

// ---- the MSM's plans against the carve-up of their workspace (msm_ws.h, zkt_msm_plan.cpp: the library's own host code) ----
#include "msm_ws.h"
namespace {
// form 0: msm_plan (resident), 1: msm_plan_direct (one-shot), 2: msm_plan_batch of k vectors
MsmPlan hostcheck_msm_plan(size_t n, int grp, int form, int k) { return form == 0 ? msm_plan(n, grp) : form == 1 ? msm_plan_direct(n, grp) : msm_plan_batch(n, grp, k); }
}  // namespace
extern "C" {
size_t zkt_hostcheck_msm_ws_bytes(size_t n, int grp, int form, int k) { return hostcheck_msm_plan(n, grp, form, k).ws_bytes; }
// The carve of that plan over a 256-byte-aligned base: returns the offset of its end, and in offs[0..27) the offset of every pointer it hands out (~0 for one it
// leaves null), in the order entries, slot, sums, order, rec, subhist (used at 256-byte alignment), then counts, cursor, size_hist, size_off, size_cur, hot,
// offsets, colsum, rowsum, clsA, clsB, win_jac, scan_tmp, ntask, task_off, partial, hot_part, tilehist, tileoff, blkoff, part_scan (words).
size_t zkt_hostcheck_msm_carve(size_t n, int grp, int form, int k, size_t* offs) {
  alignas(256) static uint8_t base[256];      // only its address is used: the carve computes pointers and touches nothing
  const MsmWs w = carve(hostcheck_msm_plan(n, grp, form, k), base);
  const void* p[] = {w.entries, w.slot, w.sums, w.order, w.rec, w.subhist, w.counts, w.cursor, w.size_hist, w.size_off, w.size_cur, w.hot, w.offsets, w.colsum, w.rowsum,
                     w.clsA, w.clsB, w.win_jac, w.scan_tmp, w.ntask, w.task_off, w.partial, w.hot_part, w.tilehist, w.tileoff, w.blkoff, w.part_scan};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) offs[i] = p[i] ? (size_t)((const uint8_t*)p[i] - base) : ~(size_t)0;
  return (size_t)(w.end - base);
}
}  // extern "C"

// ---- the layout of a host-pointer call's staging slots (host_stage.h: the library's own host code) ----
#include "host_stage.h"
extern "C" {
int zkt_hostcheck_stage_slots() { return STAGE_SLOTS; }
size_t zkt_hostcheck_stage_layout(const size_t* bytes, int count, size_t* offsets) { return stage_layout(bytes, count, offsets); }
}  // extern "C"
