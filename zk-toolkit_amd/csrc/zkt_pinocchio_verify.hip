// Pinocchio verification against a RESIDENT verification key, a batch of proofs per call — SURVEY §8 row f-4, Verifier::verify (pinocchio/verifier.rs:31-85)
// once per proof against one VerificationKeys (crs.rs:24-39).  zkt_pinocchio_verify (zkt_pinocchio.hip) decides one proof per call on the lane-distributed
// kernels (~6.5 ms, latency-bound); here a proof is five lanes of the one-element-per-lane 63-step kernels (pairing.h, "optimal ate"):
//   check  verifier.rs  pairs (G1, G2)                                                     key G2 (line table)   chain in the lane   shape <KV,KF>
//   0      :43-48       (beta_vwy_mid_s, gamma) -(v_mid_s + g1_w_mid_s + y_mid_s, beta_gamma)  gamma, beta_gamma                         <0,2>
//   1      :51-55       (alpha_v_mid_s, one_g2) -(v_mid_s, alpha_v)                            one_g2, alpha_v                           <0,2>
//   2      :56-60       (alpha_w_mid_s, one_g2) -(alpha_w, g2_w_mid_s)                         one_g2                g2_w_mid_s          <1,1>
//   3      :61-65       (alpha_y_mid_s, one_g2) -(y_mid_s, alpha_y)                            one_g2, alpha_y                           <0,2>
//   4      :68-84       (v_s, w_s) -(t, h_s) -(y_s, one_g2)                                    one_g2                w_s, h_s            <2,1>
// Seven of the eleven G2 arguments are key constants: their 68 line triples are tabulated once per key (ate_line_table), so a proof runs 3 G2 chains, reads
// 11 line streams and takes 5 final exponentiations.  Whatever does not fit the 63-step loop — a point off its curve or outside its group, or a key that
// failed its tests — is decided by the shared product-check launchers (zkt_pairing.hip) on a compacted batch, with their own 255-step / exact sequence.
#include <vector>
#include <memory>
#include <mutex>
#include <cstring>
#include "abi.h"
#include "zkt_internal.h"
#include "../../include/zkt.h"
#include "host_abi.h"

namespace zkt {
// the outcome of one check of one proof.  PIN_REDO: the check does not fit the 63-step loop, the launchers behind decide it
static constexpr uint32_t PIN_REJECT = 0, PIN_ACCEPT = 1, PIN_REDO = 2, PIN_INF = 3;
static constexpr int32_t PIN_MARKED = INT32_MIN;        // verdict of a proof whose first check that is not an accept is PIN_REDO
static constexpr uint32_t PIN_KEY_GOOD = 0x1ffu;         // every bit of the key's verdict word (k_pinocchio_key_prep)
// device views of one batch: the proof's nine arrays (n points each), the four sums k_pinocchio_sums forms, the key's points in the ABI layout
//   kg2: one_g2, alpha_v, alpha_y, gamma, beta_gamma (the order of the key's line tables);  kg1: alpha_w, t
struct PinBatch {
  const uint32_t *v, *w1, *y, *av, *aw, *ay, *b, *w2, *h;
  const uint32_t *vwy, *vs, *ys, *ws;
  const uint32_t *kg2, *kg1;
  size_t n;
};
struct PinPair { const uint32_t* p; const uint32_t* q; };
// pair k of check c of proof i in the reference's order; pairs with k > 0 stand on the right-hand side (their G1 point is negated)
__device__ inline PinPair pin_pair(const PinBatch& B, int c, int k, size_t i) {
  const uint32_t *one = B.kg2, *alpha_v = B.kg2 + ABI_G2_WORDS, *alpha_y = B.kg2 + 2 * ABI_G2_WORDS, *gamma = B.kg2 + 3 * ABI_G2_WORDS, *beta_gamma = B.kg2 + 4 * ABI_G2_WORDS;
  const size_t o1 = i * ABI_G1_WORDS, o2 = i * ABI_G2_WORDS;
  switch (c * 3 + k) {
    case 0: return PinPair{B.b + o1, gamma};
    case 1: return PinPair{B.vwy + o1, beta_gamma};
    case 3: return PinPair{B.av + o1, one};
    case 4: return PinPair{B.v + o1, alpha_v};
    case 6: return PinPair{B.aw + o1, one};
    case 7: return PinPair{B.kg1, B.w2 + o2};
    case 9: return PinPair{B.ay + o1, one};
    case 10: return PinPair{B.y + o1, alpha_y};
    case 12: return PinPair{B.vs + o1, B.ws + o2};
    case 13: return PinPair{B.kg1 + ABI_G1_WORDS, B.h + o2};
    default: return PinPair{B.ys + o1, one};
  }
}
__device__ inline int pin_pairs_of(int c) { return c == 4 ? 3 : 2; }

// ---- key preparation ----------------------------------------------------------------------------------------------------------------------------
// Once per key, in the manner of k_ate_key_prep: block 0 tabulates the lines of the five G2 points (a lane each; the table's end test says whether the point is in
// G2), block 1 tests alpha_w and t, block 2 the io points.  verdict (zeroed by the caller):
//   bits 0-4  one_g2, alpha_v, alpha_y, gamma, beta_gamma finite, on E' and in G2      bit 5 / 6  alpha_w / t finite, on E and in G1
//   bit 7     every point of vk_io and yk_io at infinity or in G1                      bit 8      every point of wk_io at infinity or in G2
__global__ void __launch_bounds__(64) k_pinocchio_key_prep(const uint32_t* __restrict__ kg2, const uint32_t* __restrict__ kg1, const uint32_t* __restrict__ io1,
                                                           const uint32_t* __restrict__ io2, int n_io, uint32_t* __restrict__ lines, uint32_t* __restrict__ verdict) {
  constexpr size_t T = (size_t)ATE_LINES * ATE_LINE_WORDS;
  const int j = threadIdx.x;
  if (blockIdx.x == 0) {
    if (j < 5) {
      const Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(kg2 + (size_t)j * ABI_G2_WORDS);
      if (!q.inf && g2_on_curve(q.x, q.y) && ate_line_table(q.x, q.y, lines + j * T)) atomicOr(verdict, 1u << j);
    }
  } else if (blockIdx.x == 1) {
    if (j < 2) {
      const Aff<FqOps> p = PtIO<FqOps>::ld(kg1 + (size_t)j * ABI_G1_WORDS);
      if (!p.inf && g1_on_curve(p.x, p.y) && g1_in_subgroup(p.x, p.y)) atomicOr(verdict, 32u << j);
    }
  } else {
    bool bad1 = false, bad2 = false;                 // infinity is the neutral element: an io point may be it
    if (j < 2 * n_io) {
      const Aff<FqOps> p = PtIO<FqOps>::ld(io1 + (size_t)j * ABI_G1_WORDS);
      bad1 = !(p.inf || (g1_on_curve(p.x, p.y) && g1_in_subgroup(p.x, p.y)));
    } else if (j < 3 * n_io) {
      const Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(io2 + (size_t)(j - 2 * n_io) * ABI_G2_WORDS);
      bad2 = !(q.inf || (g2_on_curve(q.x, q.y) && g2_in_subgroup(q.x, q.y)));
    }
    const unsigned long long b1 = __ballot(bad1), b2 = __ballot(bad2);
    if (j == 0) atomicOr(verdict, (b1 ? 0u : 128u) | (b2 ? 0u : 256u));
  }
}

// ---- statement sums, per proof ------------------------------------------------------------------------------------------------------------------------
// A batch form of k_pin_sums (zkt_pinocchio.hip): out[i] = fix_0[i] + .. + terms[0 * n + i] + .. (complete additions, one lane per output, one normalisation each).
// blockIdx.y selects the output:  G1  0: vwy = v_mid_s + g1_w_mid_s + y_mid_s (:44)   1: v_s = v_mid_s + v_io (:70-72)   2: y_s = y_mid_s + y_io (:75-76)
//                                 G2  0: w_s = g2_w_mid_s + w_io (:73-74)
struct PinSumJob { const uint32_t* fix[3]; int nfix; const uint32_t* terms; int nterms; uint32_t* out; };
struct PinSumJobs { PinSumJob j[3]; };
template <class F>
__global__ void __launch_bounds__(64) k_pinocchio_sums(PinSumJobs jobs, size_t n) {
  constexpr int W = PtIO<F>::WORDS;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const PinSumJob& q = jobs.j[blockIdx.y];
  Jac<F> acc = jac_inf<F>();
  for (int k = 0; k < q.nfix; ++k) acc = jac_add_aff(acc, PtIO<F>::ld(q.fix[k] + i * W));
  for (int t = 0; t < q.nterms; ++t) acc = jac_add_aff(acc, PtIO<F>::ld(q.terms + ((size_t)t * n + i) * W));
  PtIO<F>::st(q.out + i * W, jac_to_aff(acc));
}
// w_io of a large batch, one lane per proof: sum_j io_j * wk_io[j] from the points' 16^w tables (launch_fixed_tables) by bit planes — acc <- 2 acc, then every table
// entry whose 4-bit digit has the plane's bit set is added: 4 doublings and ~32 mixed additions per wire, where one wave per product (launch_fixed_muls_batch, the
// small batches' form) spends 64 lanes x ~15 operations.
__global__ void __launch_bounds__(64) k_pinocchio_g2_io_sums(const uint32_t* __restrict__ tab16, const uint32_t* __restrict__ io, int n_io, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Jac<Fq2Ops> acc = jac_inf<Fq2Ops>();
  for (int b = 3; b >= 0; --b) {
    acc = jac_dbl(acc);
    for (int j = 0; j < n_io; ++j) {
      const uint32_t* k = io + (i * n_io + j) * 8;
      for (int w = 0; w < 64; ++w)
        if ((k[w >> 3] >> ((w & 7) * 4 + b)) & 1u) acc = jac_add_aff(acc, PtIO<Fq2Ops>::ld(tab16 + ((size_t)j * 64 + w) * ABI_G2_WORDS));
    }
  }
  PtIO<Fq2Ops>::st(out + i * ABI_G2_WORDS, jac_to_aff(acc));
}

// ---- the five checks on the 63-step loop --------------------------------------------------------------------------------------------------------------
// Miller slot m of check c (the KV chain pairs first, then the KF table pairs):  the reference's pair index, the row of `fits` that holds the G1 argument's test
// (-1: a key point, or v_s / y_s standing in rows 3 / 6 below), and the key's line table (-1: the pair runs its chain).
// fits rows (launch_g1_fits): 0 beta_vwy_mid_s, 1 vwy, 2 alpha_v_mid_s, 3 v_mid_s, 4 alpha_w_mid_s, 5 alpha_y_mid_s, 6 y_mid_s.  v_s is in G1 exactly when v_mid_s is,
// y_s exactly when y_mid_s is: the io points were tested with the key.
__device__ const int8_t PIN_SLOT_PAIR[5][3] = {{0, 1, -1}, {0, 1, -1}, {1, 0, -1}, {0, 1, -1}, {0, 1, 2}};
__device__ const int8_t PIN_SLOT_FIT[5][3] = {{0, 1, -1}, {2, 3, -1}, {-1, 4, -1}, {5, 6, -1}, {3, -1, 6}};
__device__ const int8_t PIN_SLOT_TAB[5][3] = {{3, 4, -1}, {0, 1, -1}, {-1, 0, -1}, {0, 2, -1}, {-1, -1, 0}};
// One (proof, check) per lane, the check uniform per block: c = c_first, or for the three <0,2> checks 0, 1, 3 by blockIdx.y (each segment whole waves).
// code[c * n + i] <- PIN_INF (an argument at infinity: the reference's panic), PIN_REDO (a G1 argument that failed its test, a G2 argument off E' or outside G2),
// or the decision, compared as k_pairing_product_check_ate does.
template <int KV, int KF>
__global__ void __launch_bounds__(64) k_pinocchio_check(PinBatch B, int c_first, const uint32_t* __restrict__ lines, const uint32_t* __restrict__ fits, uint32_t* __restrict__ code) {
  constexpr int K = KV + KF;
  constexpr size_t T = (size_t)ATE_LINES * ATE_LINE_WORDS;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x, n = B.n;
  const int c = c_first + (blockIdx.y == 2 ? 3 : (int)blockIdx.y);
  if (i >= n) return;
  Fq xp[K], yp[K]; Fq2 xq[KV > 0 ? KV : 1], yq[KV > 0 ? KV : 1];
  const uint32_t* tabs[KF];
  bool inf = false, fit = true;
  for (int m = 0; m < K; ++m) {
    const int r = PIN_SLOT_PAIR[c][m], f = PIN_SLOT_FIT[c][m];
    const PinPair pr = pin_pair(B, c, r, i);
    const Aff<FqOps> p = PtIO<FqOps>::ld(pr.p);
    inf = inf || p.inf;
    xp[m] = p.x; yp[m] = r ? fp_neg(p.y) : p.y;
    if (f >= 0) fit = fit && fits[(size_t)f * n + i] != 0;
    if (m < KV) {
      const Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(pr.q);
      inf = inf || q.inf;
      xq[m] = q.x; yq[m] = q.y;
    } else tabs[m - KV] = lines + (size_t)PIN_SLOT_TAB[c][m] * T;        // the key's G2 points are finite: its verdict word
  }
  uint32_t* out = code + (size_t)c * n + i;
  if (inf) { *out = PIN_INF; return; }
  if (!fit) { *out = PIN_REDO; return; }
  for (int m = 0; m < KV; ++m) if (!g2_on_curve(xq[m], yq[m])) { *out = PIN_REDO; return; }
  bool in_g2;
  const Fq12 f = miller_ate_multi<KV, KF>(xp, yp, xq, yq, tabs, in_g2);
  if (!in_g2) { *out = PIN_REDO; return; }
  uint32_t got[144]; st_fq12(got, final_exponentiation_3h(f));      // three times the exact exponent: decisions only (pairing.h)
  uint32_t diff = got[132] ^ 1u;                                     // canonical one: w0.v0.u0 = 1, all else 0
  for (int k = 0; k < 144; ++k) if (k != 132) diff |= got[k];
  *out = diff == 0 ? PIN_ACCEPT : PIN_REJECT;
}
// A key that failed its tests: no check fits.  code <- PIN_INF where an argument is at infinity (the key's points included), else PIN_REDO.
__global__ void __launch_bounds__(64) k_pinocchio_classify(PinBatch B, uint32_t* __restrict__ code) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= B.n) return;
  bool inf = false;
  for (int k = 0; k < pin_pairs_of(c); ++k) { const PinPair pr = pin_pair(B, c, k, i); inf = inf || pr.p[2 * FqC::ABI_N] != 0 || pr.q[48] != 0; }
  code[(size_t)c * B.n + i] = inf ? PIN_INF : PIN_REDO;
}
// Small batches: element e = c * n + i of launch_pairing_product_check_counts, three pair slots each (the two-pair checks repeat their pair 0 in slot 2, as
// pin_verify_fast packs them for n = 1).  That launcher has ONE error word for all its elements, so which elements have an argument at infinity is noted here.
__global__ void __launch_bounds__(64) k_pinocchio_pack(PinBatch B, uint32_t* __restrict__ g1, uint32_t* __restrict__ g2, uint8_t* __restrict__ kcount, uint32_t* __restrict__ isinf) {
  const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= 5 * B.n) return;
  const int c = (int)(e / B.n); const size_t i = e % B.n;
  const int kc = pin_pairs_of(c);
  bool inf = false;
  for (int k = 0; k < 3; ++k) {
    const PinPair pr = pin_pair(B, c, k < kc ? k : 0, i);
    uint32_t* o1 = g1 + (e * 3 + k) * ABI_G1_WORDS; uint32_t* o2 = g2 + (e * 3 + k) * ABI_G2_WORDS;
    for (int w = 0; w < ABI_G1_WORDS; ++w) o1[w] = pr.p[w];
    for (int w = 0; w < ABI_G2_WORDS; ++w) o2[w] = pr.q[w];
    inf = inf || pr.p[2 * FqC::ABI_N] != 0 || pr.q[48] != 0;
  }
  kcount[e] = (uint8_t)kc; isinf[e] = inf ? 1u : 0u;
}
// verdict[i] from the five codes of proof i in the reference's order (verifier.rs:43-84): the first check that is not an accept decides — reject -> 0, infinity ->
// -ZKT_ERR_INFINITY, PIN_REDO -> the proof is marked (and counted) for the launchers behind.  isinf (small batches): code = the product kernel's ok, PIN_INF where noted.
__global__ void __launch_bounds__(256) k_pinocchio_decide(uint32_t* __restrict__ code, const uint32_t* __restrict__ isinf, size_t n, int32_t* __restrict__ verdict, uint32_t* __restrict__ marked) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t v = 1;
  for (int c = 4; c >= 0; --c) {
    uint32_t cd = code[(size_t)c * n + i];
    if (isinf && isinf[(size_t)c * n + i]) { cd = PIN_INF; code[(size_t)c * n + i] = cd; }
    if (cd != PIN_ACCEPT) v = cd == PIN_REJECT ? 0 : cd == PIN_INF ? -ZKT_ERR_INFINITY : PIN_MARKED;      // descending: the earliest check has the last word
  }
  verdict[i] = v;
  if (v == PIN_MARKED) atomicAdd(marked, 1u);
}
// The compacted batch of the launchers behind: element j is (proof, check) e = idx[j], its K pairs copied to slot-major arrays g1[k * m + j], g2[k * m + j].
__global__ void __launch_bounds__(64) k_pinocchio_gather(PinBatch B, const unsigned long long* __restrict__ idx, size_t m, int K, uint32_t* __restrict__ g1, uint32_t* __restrict__ g2) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= m * (size_t)K) return;
  const int k = (int)(t / m); const size_t j = t % m;
  const size_t e = (size_t)idx[j];
  const PinPair pr = pin_pair(B, (int)(e / B.n), k, e % B.n);
  uint32_t* o1 = g1 + t * ABI_G1_WORDS; uint32_t* o2 = g2 + t * ABI_G2_WORDS;
  for (int w = 0; w < ABI_G1_WORDS; ++w) o1[w] = pr.p[w];
  for (int w = 0; w < ABI_G2_WORDS; ++w) o2[w] = pr.q[w];
}
// The product-check launchers report the reference's panics on ITS chain (a multiple of P at infinity, a vanishing denominator: points outside G1) through one
// error word per launch.  When that word is set, this kernel says which of the rejected elements are panics: the reference's chain once more, lines only.
__global__ void __launch_bounds__(64) k_pinocchio_exact_panics(PairArgs a, int K, const uint32_t* __restrict__ ok, uint32_t* __restrict__ panic, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || ok[i] != 0) return;
  for (int k = 0; k < K; ++k) {
    const Aff<FqOps> p = PtIO<FqOps>::ld(a.g1[k] + i * a.s1[k]);
    const Aff<Fq2Ops> q = PtIO<Fq2Ops>::ld(a.g2[k] + i * a.s2[k]);
    bool bad;
    (void)miller_g1_g2_exact(p.x, p.y, q.x, q.y, bad);
    if (bad) { panic[i] = 1; return; }
  }
}
}  // namespace zkt

using namespace zkt;

struct zkt_pinocchio_vk {
  size_t n_io = 0;
  uint32_t key_verdict = 0;                         // k_pinocchio_key_prep; PIN_KEY_GOOD: the 63-step kernels serve this key
  // device memory, owned by the handle (zkt_shutdown does not touch it; zkt_pinocchio_vk_free releases it)
  Dev lines;                                        // 5 x ATE_LINES * ATE_LINE_WORDS words + the verdict word
  Dev kg2, kg1;                                     // one_g2, alpha_v, alpha_y, gamma, beta_gamma | alpha_w, t (ABI layout)
  Dev io1, io2;                                     // [vk_io | yk_io], wk_io (ABI layout)
  Dev tab1, tab2;                                   // their 16^w tables (launch_fixed_tables): small batches' statement products, and the G2 bit-plane sums
  Dev wide;                                         // 8-bit window tables of vk_io, then of yk_io (launch_stmt_wide_tables): large batches' G1 statement sums
  std::mutex mu;                                    // a handle serves one call at a time
};

namespace {
constexpr size_t PIN_MAX_IO = 12;                   // launch_fixed_tables and launch_stmt_wide_tables take twelve points
constexpr size_t LINE_T = (size_t)ATE_LINES * ATE_LINE_WORDS;
constexpr int W1 = ABI_G1_WORDS, W2 = ABI_G2_WORDS;

// the checks marked PIN_REDO of the marked proofs, on the shared launchers: K = 2 over the two-pair checks, K = 3 over the divisibility check.  code <- their decisions.
int pin_general_route(const PinBatch& B, std::vector<uint32_t>& code, const std::vector<int32_t>& verdict, hipStream_t s) {
  const size_t n = B.n;
  for (int K = 2; K <= 3; ++K) {
    std::vector<unsigned long long> idx;
    for (int c = (K == 2 ? 0 : 4); c < (K == 2 ? 4 : 5); ++c)
      for (size_t i = 0; i < n; ++i) if (verdict[i] == PIN_MARKED && code[(size_t)c * n + i] == PIN_REDO) idx.push_back((unsigned long long)c * n + i);
    const size_t m = idx.size();
    if (!m) continue;
    Dev didx(m * 8, true), g1(m * K * G1B, true), g2(m * K * G2B, true), dok(m * 4, true), derr(8, true), dpanic(m * 4, true);
    if (!didx.p || !g1.p || !g2.p || !dok.p || !derr.p || !dpanic.p) return ZKT_ERR_DEVICE;
    const unsigned long long noerr = NO_ERR;
    HIPCHK(hipMemcpyAsync(didx.p, idx.data(), m * 8, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(derr.p, &noerr, 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dok.p, 0, m * 4, s));
    hipLaunchKernelGGL(k_pinocchio_gather, dim3(grid_blocks(m * K, 64)), dim3(64), 0, s, B, (const unsigned long long*)didx.p, m, K, g1.w(), g2.w());
    HIPCHK(hipGetLastError());
    PairArgs a{};
    for (int k = 0; k < K; ++k) { a.g1[k] = g1.w() + (size_t)k * m * W1; a.g2[k] = g2.w() + (size_t)k * m * W2; a.s1[k] = W1; a.s2[k] = W2; a.neg[k] = k ? 1 : 0; }
    HIPCHK(launch_pairing_product_check(a, K, dok.w(), m, (unsigned long long*)derr.p, s));
    std::vector<uint32_t> ok(m), panic(m, 0); unsigned long long e = NO_ERR;
    HIPCHK(hipMemcpyAsync(ok.data(), dok.p, m * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&e, derr.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (e != NO_ERR) {                                // no element here has an argument at infinity: a panic on the reference's own chain
      HIPCHK(hipMemsetAsync(dpanic.p, 0, m * 4, s));
      hipLaunchKernelGGL(k_pinocchio_exact_panics, dim3(grid_blocks(m, 64)), dim3(64), 0, s, a, K, (const uint32_t*)dok.w(), dpanic.w(), m);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(panic.data(), dpanic.p, m * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    for (size_t j = 0; j < m; ++j) code[(size_t)idx[j]] = panic[j] ? PIN_INF : ok[j] == 1 ? PIN_ACCEPT : PIN_REJECT;
  }
  return ZKT_OK;
}
// the order rule of pin_decide (zkt_pinocchio.hip) on five decided codes
int32_t pin_fold(const std::vector<uint32_t>& code, size_t n, size_t i) {
  for (int c = 0; c < 5; ++c) {
    const uint32_t cd = code[(size_t)c * n + i];
    if (cd == PIN_INF) return -ZKT_ERR_INFINITY;
    if (cd != PIN_ACCEPT) return 0;
  }
  return 1;
}
}  // namespace

extern "C" {

int zkt_pinocchio_vk_create(const zkt_pinocchio_crs* c, zkt_pinocchio_vk** out) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!c || !out || !c->one_g2 || !c->alpha_v || !c->alpha_w || !c->alpha_y || !c->gamma || !c->beta_gamma || !c->t) return ZKT_ERR_SHAPE;
  const size_t nio = c->n_io;
  if (nio > PIN_MAX_IO || (nio && (!c->vk_io || !c->wk_io || !c->yk_io))) return ZKT_ERR_SHAPE;
  std::unique_ptr<zkt_pinocchio_vk> vk(new zkt_pinocchio_vk);
  vk->n_io = nio;
  hipStream_t s = nullptr;
  const zkt_g2_affine kg2[5] = {*c->one_g2, *c->alpha_v, *c->alpha_y, *c->gamma, *c->beta_gamma};
  const zkt_g1_affine kg1[2] = {*c->alpha_w, *c->t};
  if (vk->lines.alloc((5 * LINE_T + 2) * 4) || vk->kg2.alloc(sizeof kg2) || vk->kg1.alloc(sizeof kg1) || vk->io1.alloc(2 * nio * G1B) || vk->io2.alloc(nio * G2B) ||
      vk->tab1.alloc(2 * nio * 64 * G1B) || vk->tab2.alloc(nio * 64 * G2B) || vk->wide.alloc(nio ? 2 * stmt_wide_table_words((int)nio) * 4 : 0)) return ZKT_ERR_DEVICE;
  uint32_t* dverdict = vk->lines.w() + 5 * LINE_T;
  ZCHK(up(vk->kg2, kg2, sizeof kg2, s)); ZCHK(up(vk->kg1, kg1, sizeof kg1, s));
  HIPCHK(hipMemsetAsync(vk->lines.p, 0, (5 * LINE_T + 2) * 4, s));
  if (nio) {
    HIPCHK(hipMemcpyAsync(vk->io1.p, c->vk_io, nio * G1B, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(vk->io1.w() + nio * W1, c->yk_io, nio * G1B, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(vk->io2.p, c->wk_io, nio * G2B, hipMemcpyHostToDevice, s));
    for (int half = 0; half < 2; ++half) {
      FixedTables ft{}; ft.n = (int)nio;
      for (size_t j = 0; j < nio; ++j) { ft.point[j] = vk->io1.w() + (half * nio + j) * W1; ft.table[j] = vk->tab1.w() + (half * nio + j) * 64 * W1; }
      HIPCHK(launch_fixed_tables(G_G1, ft, s));
    }
    FixedTables ft{}; ft.n = (int)nio;
    for (size_t j = 0; j < nio; ++j) { ft.point[j] = vk->io2.w() + j * W2; ft.table[j] = vk->tab2.w() + j * 64 * W2; }
    HIPCHK(launch_fixed_tables(G_G2, ft, s));
    for (int half = 0; half < 2; ++half)
      HIPCHK(launch_stmt_wide_tables(vk->tab1.w() + half * nio * 64 * W1, (int)nio, vk->wide.w() + half * stmt_wide_table_words((int)nio), s));
  }
  hipLaunchKernelGGL(k_pinocchio_key_prep, dim3(3), dim3(64), 0, s, (const uint32_t*)vk->kg2.w(), (const uint32_t*)vk->kg1.w(), (const uint32_t*)vk->io1.w(),
                     (const uint32_t*)vk->io2.w(), (int)nio, vk->lines.w(), dverdict);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&vk->key_verdict, dverdict, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *out = vk.release();
  return ZKT_OK;
}
void zkt_pinocchio_vk_free(zkt_pinocchio_vk* vk) { delete vk; }

}  // extern "C"
namespace {
// n proofs through one route.  Caller holds vk->mu.
int pin_verify_some(zkt_pinocchio_vk* vk, const zkt_pinocchio_proof* pf, const uint64_t* io_wires, size_t n, int32_t* verdict) {
  hipStream_t s = nullptr;                          // the stream every protocol call uses (scratch budget: DESIGN.md §4)
  const size_t nio = vk->n_io;
  const bool key_good = vk->key_verdict == PIN_KEY_GOOD;
  bool small = key_good && 15 * n <= dproduct_limit();
  // the proof's arrays: seven G1 (v, w1, y, av, aw, ay, b), two G2 (w2, h); behind them the sums vwy, v_s, y_s | w_s
  Dev d1(10 * n * G1B, true), d2(3 * n * G2B, true), dio(n * nio * FRB, true), dcode(5 * n * 4, true), dverdict(n * 4, true), dmarked(4, true);
  if (!d1.p || !d2.p || !dio.p || !dcode.p || !dverdict.p || !dmarked.p) return ZKT_ERR_DEVICE;
  const zkt_g1_affine* h1[7] = {pf->v_mid_s, pf->g1_w_mid_s, pf->y_mid_s, pf->alpha_v_mid_s, pf->alpha_w_mid_s, pf->alpha_y_mid_s, pf->beta_vwy_mid_s};
  const zkt_g2_affine* h2[2] = {pf->g2_w_mid_s, pf->h_s};
  for (int k = 0; k < 7; ++k) HIPCHK(hipMemcpyAsync(d1.w() + (size_t)k * n * W1, h1[k], n * G1B, hipMemcpyHostToDevice, s));
  for (int k = 0; k < 2; ++k) HIPCHK(hipMemcpyAsync(d2.w() + (size_t)k * n * W2, h2[k], n * G2B, hipMemcpyHostToDevice, s));
  if (nio) HIPCHK(hipMemcpyAsync(dio.p, io_wires, n * nio * FRB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(dmarked.p, 0, 4, s));
  auto A1 = [&](int k) { return d1.w() + (size_t)k * n * W1; };
  auto A2 = [&](int k) { return d2.w() + (size_t)k * n * W2; };
  PinBatch B{A1(0), A1(1), A1(2), A1(3), A1(4), A1(5), A1(6), A2(0), A2(1), A1(7), A1(8), A1(9), A2(2), vk->kg2.w(), vk->kg1.w(), n};
  // statement sums (verifier.rs:70-76).  Small batches: one wave per product from the 16^w tables; large ones: one lane per proof (8-bit windows in G1, bit planes in G2)
  {
    Dev t1, t2;
    int nt1 = 0, nt2 = 0;
    if (nio) {
      if (small) {
        if (t1.alloc(2 * nio * n * G1B, true) || t2.alloc(nio * n * G2B, true)) return ZKT_ERR_DEVICE;
        HIPCHK(launch_fixed_muls_batch(G_G1, vk->tab1.w(), dio.w(), t1.w(), n, (int)nio, s));
        HIPCHK(launch_fixed_muls_batch(G_G1, vk->tab1.w() + nio * 64 * W1, dio.w(), t1.w() + nio * n * W1, n, (int)nio, s));
        HIPCHK(launch_fixed_muls_batch(G_G2, vk->tab2.w(), dio.w(), t2.w(), n, (int)nio, s));
        nt1 = nt2 = (int)nio;
      } else {
        if (t1.alloc(2 * n * G1B, true) || t2.alloc(n * G2B, true)) return ZKT_ERR_DEVICE;
        for (int half = 0; half < 2; ++half)
          HIPCHK(launch_stmt_sums_wide(vk->wide.w() + half * stmt_wide_table_words((int)nio), dio.w(), (int)nio, t1.w() + (size_t)half * n * W1, n, s));
        hipLaunchKernelGGL(k_pinocchio_g2_io_sums, dim3(grid_blocks(n, 64)), dim3(64), 0, s, (const uint32_t*)vk->tab2.w(), (const uint32_t*)dio.w(), (int)nio, t2.w(), n);
        nt1 = nt2 = 1;
      }
    }
    PinSumJobs j1{}, j2{};
    j1.j[0] = PinSumJob{{B.v, B.w1, B.y}, 3, nullptr, 0, A1(7)};
    j1.j[1] = PinSumJob{{B.v, nullptr, nullptr}, 1, t1.w(), nt1, A1(8)};
    j1.j[2] = PinSumJob{{B.y, nullptr, nullptr}, 1, t1.w() ? t1.w() + (size_t)nt1 * n * W1 : nullptr, nt1, A1(9)};
    j2.j[0] = PinSumJob{{B.w2, nullptr, nullptr}, 1, t2.w(), nt2, A2(2)};
    hipLaunchKernelGGL(k_pinocchio_sums<FqOps>, dim3(grid_blocks(n, 64), 3), dim3(64), 0, s, j1, n);
    hipLaunchKernelGGL(k_pinocchio_sums<Fq2Ops>, dim3(grid_blocks(n, 64), 1), dim3(64), 0, s, j2, n);
    HIPCHK(hipGetLastError());
  }
  const dim3 g64(grid_blocks(n, 64));
  bool decided = false;
  if (small) {
    // 5 n elements x 3 pair slots on the lane-distributed kernels, as pin_verify_fast does for n = 1
    Dev p1(15 * n * G1B, true), p2(15 * n * G2B, true), dcnt(5 * n, true), dinf(5 * n * 4, true), derr(8, true);
    if (!p1.p || !p2.p || !dcnt.p || !dinf.p || !derr.p) return ZKT_ERR_DEVICE;
    const unsigned long long noerr = NO_ERR;
    HIPCHK(hipMemcpyAsync(derr.p, &noerr, 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pinocchio_pack, dim3(grid_blocks(5 * n, 64)), dim3(64), 0, s, B, p1.w(), p2.w(), (uint8_t*)dcnt.p, dinf.w());
    HIPCHK(hipGetLastError());
    PairArgs a{};
    for (int j = 0; j < 3; ++j) { a.g1[j] = p1.w() + j * W1; a.g2[j] = p2.w() + j * W2; a.s1[j] = 3 * W1; a.s2[j] = 3 * W2; a.neg[j] = j ? 1 : 0; }
    const hipError_t le = launch_pairing_product_check_counts(a, 3, (const uint8_t*)dcnt.p, dcode.w(), 5 * n, (unsigned long long*)derr.p, s);
    if (le == hipErrorInvalidValue) (void)hipGetLastError();      // the small-batch kernels are switched off (ZKT_DPRODUCT_MAX): the one-proof-per-lane kernels below
    else {
      HIPCHK(le);
      hipLaunchKernelGGL(k_pinocchio_decide, dim3(grid_blocks(n)), dim3(256), 0, s, dcode.w(), (const uint32_t*)dinf.w(), n, (int32_t*)dverdict.p, dmarked.w());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s));              // the packed arrays are released behind this block
      decided = true;
    }
  }
  if (!decided) {
    if (key_good) {
      // membership of the seven per-proof G1 arguments at four waves per SIMD (launch_g1_fits, K <= 4 arrays per launch), then the three shapes
      Dev fits(7 * n * 4, true);
      if (!fits.p) return ZKT_ERR_DEVICE;
      G1Fits fa{}, fb{};
      const uint32_t* rows[7] = {B.b, B.vwy, B.av, B.v, B.aw, B.ay, B.y};
      for (int k = 0; k < 4; ++k) { fa.pts[k] = rows[k]; fa.stride[k] = W1; }
      for (int k = 0; k < 3; ++k) { fb.pts[k] = rows[4 + k]; fb.stride[k] = W1; }
      HIPCHK(launch_g1_fits(fa, 4, fits.w(), n, s)); HIPCHK(launch_g1_fits(fb, 3, fits.w() + 4 * n, n, s));
      const uint32_t* lines = vk->lines.w(); const uint32_t* f = fits.w();
      hipLaunchKernelGGL((k_pinocchio_check<0, 2>), dim3(g64.x, 3), dim3(64), 0, s, B, 0, lines, f, dcode.w());
      hipLaunchKernelGGL((k_pinocchio_check<1, 1>), g64, dim3(64), 0, s, B, 2, lines, f, dcode.w());
      hipLaunchKernelGGL((k_pinocchio_check<2, 1>), g64, dim3(64), 0, s, B, 4, lines, f, dcode.w());
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_pinocchio_decide, dim3(grid_blocks(n)), dim3(256), 0, s, dcode.w(), (const uint32_t*)nullptr, n, (int32_t*)dverdict.p, dmarked.w());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s));
    } else {
      hipLaunchKernelGGL(k_pinocchio_classify, dim3(g64.x, 5), dim3(64), 0, s, B, dcode.w());
      hipLaunchKernelGGL(k_pinocchio_decide, dim3(grid_blocks(n)), dim3(256), 0, s, dcode.w(), (const uint32_t*)nullptr, n, (int32_t*)dverdict.p, dmarked.w());
      HIPCHK(hipGetLastError());
    }
  }
  uint32_t marked = 0;
  std::vector<int32_t> v(n);
  HIPCHK(hipMemcpyAsync(v.data(), dverdict.p, n * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&marked, dmarked.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (marked) {
    std::vector<uint32_t> code(5 * n);
    HIPCHK(hipMemcpyAsync(code.data(), dcode.p, 5 * n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ZCHK(pin_general_route(B, code, v, s));
    for (size_t i = 0; i < n; ++i) if (v[i] == PIN_MARKED) v[i] = pin_fold(code, n, i);
  }
  memcpy(verdict, v.data(), n * 4);
  return ZKT_OK;
}
// Where the two routes cross, measured (profiles/pinocchio_verify_batch_timing.md): the lane-distributed kernels cost ~31 us per proof, the one-proof-per-lane kernels
// 86 ms for anything up to 4,096 proofs, so the former win below ~2,700 proofs.  launch_pairing_product_check_counts takes 15 n <= dproduct_limit() elements x slots
// (n <= 1,638 by default): a batch up to PIN_SMALL_MAX that is at most two such pieces is verified piece by piece.
constexpr size_t PIN_SMALL_MAX = 2560;
}  // namespace

extern "C" {

int zkt_pinocchio_verify_batch(zkt_pinocchio_vk* vk, const zkt_pinocchio_proof* pf, const uint64_t* io_wires, size_t n, int32_t* verdict) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!vk || !verdict) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  if (!pf || !pf->v_mid_s || !pf->g1_w_mid_s || !pf->g2_w_mid_s || !pf->y_mid_s || !pf->h_s || !pf->alpha_v_mid_s || !pf->alpha_w_mid_s || !pf->alpha_y_mid_s ||
      !pf->beta_vwy_mid_s || (vk->n_io && !io_wires) || n > (size_t(1) << 26)) return ZKT_ERR_SHAPE;
  std::lock_guard<std::mutex> lk(vk->mu);
  const size_t piece = dproduct_limit() / 15;
  if (vk->key_verdict != PIN_KEY_GOOD || n <= piece || n > PIN_SMALL_MAX || n > 2 * piece) return pin_verify_some(vk, pf, io_wires, n, verdict);
  for (size_t i0 = 0; i0 < n; i0 += piece) {
    const zkt_pinocchio_proof part = {pf->v_mid_s + i0, pf->g1_w_mid_s + i0, pf->g2_w_mid_s + i0, pf->y_mid_s + i0, pf->h_s + i0, pf->alpha_v_mid_s + i0, pf->alpha_w_mid_s + i0,
                                      pf->alpha_y_mid_s + i0, pf->beta_vwy_mid_s + i0};
    ZCHK(pin_verify_some(vk, &part, io_wires ? io_wires + i0 * vk->n_io * 4 : nullptr, n - i0 < piece ? n - i0 : piece, verdict + i0));
  }
  return ZKT_OK;
}

}  // extern "C"
