// Stand-alone check of the paired Fq products and of the paired mixed addition of the G1 accumulate loop (fp.h, curve.h) through the host entry points of csrc/hostcheck_acc_pairs.h
// (the part of csrc/hostcheck.cpp that covers them), for a host build under the address and undefined-behaviour sanitizers: tests/test_acc_pairs_hostcheck.py compiles and runs it; exit
// status 0 = every check held.  The values are compared with the unpaired products and with the Jacobian mixed addition, which tests/test_hostcheck.py holds
// against the oracle.
#include <cstdio>
#include <cstring>
#include "hostcheck_acc_pairs.h"
#include "host_abi.h"
using namespace zkt;
using zkt_hostcheck_acc_pairs::zkt_hostcheck_fq_pair;
using zkt_hostcheck_acc_pairs::zkt_hostcheck_g1_acc;

static uint64_t lcg = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 32); }
static void rand_fq(uint32_t* w) { for (int i = 0; i < 12; ++i) w[i] = rnd(); w[11] &= 0x00ffffffu; }      // below 2^376 < p
static bool same(const uint32_t* a, const uint32_t* b, int n) { for (int i = 0; i < n; ++i) if (a[i] != b[i]) return false; return true; }
static void mul(const uint32_t* a, const uint32_t* b, uint32_t* o) { st_fp<FqC>(o, fp_mul(ld_fp<FqC>(a), ld_fp<FqC>(b))); }
static void add_pts(const uint32_t* a, const uint32_t* b, uint32_t* o) { PtIO<FqOps>::st(o, jac_to_aff(jac_add_aff(jac_from_aff(PtIO<FqOps>::ld(a)), PtIO<FqOps>::ld(b)))); }

int main() {
  int bad = 0;
  uint32_t a[12], b[12], c[12], d[12], o0[12], o1[12], w0[12], w1[12];
  for (int t = 0; t < 400; ++t) {
    rand_fq(a); rand_fq(b); rand_fq(c); rand_fq(d);
    if (t < 8) for (int i = 0; i < 12; ++i) { a[i] = (i == 0) ? (uint32_t)(t & 1) : 0; c[i] = (i == 0) ? (uint32_t)(t >> 1) : 0; }
    const unsigned lifts = (unsigned)t & 255u;
    mul(a, b, w0); mul(c, d, w1);
    bad += zkt_hostcheck_fq_pair(0, a, b, c, d, lifts, o0, o1); bad += !same(o0, w0, 12) + !same(o1, w1, 12);
    bad += zkt_hostcheck_fq_pair(2, a, b, c, d, lifts, o0, o1); bad += !same(o0, w0, 12) + !same(o1, w1, 12);
    mul(a, a, w0); mul(c, c, w1);
    bad += zkt_hostcheck_fq_pair(1, a, b, c, d, lifts, o0, o1); bad += !same(o0, w0, 12) + !same(o1, w1, 12);
    bad += zkt_hostcheck_fq_pair(3, a, b, c, d, lifts, o0, o1); bad += !same(o0, w0, 12) + !same(o1, w1, 12);
  }
  // points: small multiples of the generator; every mode and sign against negate-then-add through the Jacobian formulas
  uint32_t gen[26], pts[6][26], ng[6][26], lam[12] = {7}, got[26], want[26];
  static_assert(sizeof(G1_GEN) == sizeof(gen), "one ABI point");
  std::memcpy(gen, &G1_GEN, sizeof(gen));
  for (int i = 0; i < 6; ++i) {
    const uint32_t k[1] = {(uint32_t)(i < 2 ? 3 : 3 + 5 * i)};          // pts[0] == pts[1]: the doubling exit
    Aff<FqOps> p = jac_to_aff(scalar_mul_aff(PtIO<FqOps>::ld(gen), k, 1));
    PtIO<FqOps>::st(pts[i], p);
    p.y = fp_neg(p.y); PtIO<FqOps>::st(ng[i], p);
  }
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) for (int signs = 0; signs < 4; ++signs) for (int mode = 1; mode < 3; ++mode) {
    add_pts((signs & 1) ? ng[i] : pts[i], (signs & 2) ? ng[j] : pts[j], want);
    if (zkt_hostcheck_g1_acc(mode, pts[i], pts[j], signs, lam, got) != 0 || !same(got, want, 26)) { ++bad; std::printf("point case %d %d signs %d mode %d differs\n", i, j, signs, mode); }
  }
  std::printf(bad ? "acc_pairs FAILED: %d\n" : "acc_pairs ok\n", bad);
  return bad ? 1 : 0;
}
