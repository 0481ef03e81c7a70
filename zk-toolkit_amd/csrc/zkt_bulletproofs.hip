// Bulletproofs over secp256k1, orchestrated on the device (row a18 of SURVEY §8): inner-product argument and range proof, src/zk/wo_trusted_setup/bulletproofs.rs:19-55, 58-147.
// Random values the reference draws from OS entropy (the range proof's scalars, the IPA challenges) are arguments.  secp-n scalar algebra runs in small kernels here; every
// group operation goes through the batched kernels of zkt_group.hip / zkt_msm.hip.  Host code only moves buffers and sequences launches.
#include <vector>
#include <mutex>
#include <cstring>
#include <memory>
#include "fr_vec.h"
#include "host_abi.h"

namespace zkt {
// IPA scalar stage of one level: out2 = [x, x^-1], sq2 = [x^2, x^-2], canonical
__global__ void k_ipa_challenge(const uint32_t* __restrict__ x, uint32_t* __restrict__ out2, uint32_t* __restrict__ sq2) {
  typedef SnC C;
  if (threadIdx.x || blockIdx.x) return;
  Fp<C> xm = ld_fp<C>(x), xi = fp_inv(xm), x2 = fp_sqr(xm), x2i = fp_sqr(xi);      // (x^2)^-1 = (x^-1)^2: one inversion
  st_fp<C>(out2, xm); st_fp<C>(out2 + 8, xi);
  st_fp<C>(sq2, x2); st_fp<C>(sq2 + 8, x2i);
}
// The inner-product argument over the ORIGINAL generators.  After j folds (bulletproofs.rs:44-45) the generator at folded index i is
//   gg^(j)[i] = sum_{k = i mod n_j} wG[k] gg[k],  wG[k] = prod_l (bit_l(k) ? x_l : x_l^-1)   (hh: the inverse factors),
// so L and R of every level (:39-40) are two multi-scalar multiplications over the fixed base set [gg | hh | u] with the scalars
// a^(j)[..] wG[k], b^(j)[..] wH[k] — each original generator enters exactly one of L, R — and no generator is ever folded.
// All vectors hold canonical residues (fp_mul(ld_fp(s), ld_raw(v)) = s v, as in k_fold).
// wH0 (optional): the hh generators of the argument are wH0[k] * hh[k] (the range proof's hh' = hh * y^-i, bulletproofs.rs:109, never materialised)
__global__ void __launch_bounds__(256) k_ipa_w_init(size_t N, const uint32_t* __restrict__ wH0, uint32_t* __restrict__ wG, uint32_t* __restrict__ wH) {
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k >= N) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) { wG[k * 8 + j] = j == 0; wH[k * 8 + j] = wH0 ? wH0[k * 8 + j] : (j == 0); }
}
// sL, sR: 2N+1 scalars each for the base set [gg | hh | u];  L = gg_hi*a_lo + hh_lo*b_hi + u cL,  R = gg_lo*a_hi + hh_hi*b_lo + u cR
__global__ void __launch_bounds__(256) k_ipa_level_scalars(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ wG,
                                                           const uint32_t* __restrict__ wH, const uint32_t* __restrict__ cLR, size_t N, size_t n,
                                                           uint32_t* __restrict__ sL, uint32_t* __restrict__ sR) {
  typedef SnC C;
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k > N) return;
  if (k == N) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { sL[2 * N * 8 + j] = cLR[j]; sR[2 * N * 8 + j] = cLR[8 + j]; }
    return;
  }
  const size_t np = n / 2, i = k & (n - 1); const bool hi = i >= np; const size_t j = hi ? i - np : i;
  const Fp<C> zero = fp_zero<C>();
  const Fp<C> sg = fp_mul(ld_fp<C>(a + (hi ? j : np + j) * 8), ld_raw<C>(wG + k * 8));
  const Fp<C> sh = fp_mul(ld_fp<C>(b + (hi ? j : np + j) * 8), ld_raw<C>(wH + k * 8));
  st_raw<C>(sL + k * 8, hi ? sg : zero);        st_raw<C>(sR + k * 8, hi ? zero : sg);
  st_raw<C>(sL + (N + k) * 8, hi ? zero : sh);  st_raw<C>(sR + (N + k) * 8, hi ? sh : zero);
}
// gg' = gg_lo x^-1 + gg_hi x,  hh' = hh_lo x + hh_hi x^-1  (:44-45) on the coefficient vectors
__global__ void __launch_bounds__(256) k_ipa_w_fold(const uint32_t* __restrict__ X, const uint32_t* __restrict__ XI, size_t N, size_t n,
                                                    uint32_t* __restrict__ wG, uint32_t* __restrict__ wH) {
  typedef SnC C;
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k >= N) return;
  const bool hi = (k & (n - 1)) >= n / 2;
  const Fp<C> x = ld_fp<C>(X), xi = ld_fp<C>(XI);
  st_raw<C>(wG + k * 8, fp_mul(hi ? x : xi, ld_raw<C>(wG + k * 8)));
  st_raw<C>(wH + k * 8, fp_mul(hi ? xi : x, ld_raw<C>(wH + k * 8)));
}
// base case (:28-32): g a + h b + u (a b) with g = sum wG[k] gg[k], h = sum wH[k] hh[k]
__global__ void __launch_bounds__(256) k_ipa_final_scalars(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ wG,
                                                           const uint32_t* __restrict__ wH, size_t N, uint32_t* __restrict__ sF) {
  typedef SnC C;
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k > N) return;
  const Fp<C> am = ld_fp<C>(a), bm = ld_fp<C>(b);
  if (k == N) { st_raw<C>(sF + 2 * N * 8, fp_mul(am, ld_raw<C>(b))); return; }
  st_raw<C>(sF + k * 8, fp_mul(am, ld_raw<C>(wG + k * 8)));
  st_raw<C>(sF + (N + k) * 8, fp_mul(bm, ld_raw<C>(wH + k * 8)));
}
// ---- verdict-only inner-product argument (no trace requested) ---------------------------------------------------------------------------
// The reference's function returns a bool (bulletproofs.rs:19-55); L_j and R_j are internal.  Without a trace only the verdict P_final == g a + h b + u c is observable,
// and P_final = P + sum_j (x_j^2 L_j + x_j^-2 R_j) (:47) is itself an MSM over the base set, so with sL_j, sR_j, sF the scalar vectors of the kernels above the verdict is
//   MSM_{[gg|hh|u]}( sF - sum_j (x_j^2 sL_j + x_j^-2 sR_j) ) == P
// — ONE multi-scalar multiplication, no point multiplication after the last level.  Its scalar vector needs, per original generator k and level j, one element of the
// folded a^(j), b^(j) and the running coefficient products wG, wH, so: all challenges up front (one inversion each, in parallel), the fold chain a^(j), b^(j)
// alone on the critical path (levels below 2048 elements in one block), ONE kernel over the generators that walks all levels with wG, wH in
// registers, and the 2*levels dot products for the u entry side by side.  33 MSMs and ~130 dependent launches become 1 MSM and ~12 launches.
// challenges: out[j] = {x_j, x_j^-1, x_j^2, x_j^-2} canonical
__global__ void __launch_bounds__(64) k_ipa_challenges_all(const uint32_t* __restrict__ xs, int levels, uint32_t* __restrict__ out) {
  typedef SnC C;
  const int j = blockIdx.x * 64 + threadIdx.x; if (j >= levels) return;
  Fp<C> xm = ld_fp<C>(xs + j * 8), xi = fp_inv(xm);
  st_fp<C>(out + j * 32, xm); st_fp<C>(out + j * 32 + 8, xi); st_fp<C>(out + j * 32 + 16, fp_sqr(xm)); st_fp<C>(out + j * 32 + 24, fp_sqr(xi));
}
// a' = a_lo x + a_hi x^-1, b' = b_lo x^-1 + b_hi x (:49-50) for one level, both vectors in one launch
__global__ void __launch_bounds__(256) k_ipa_fold_ab(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ ch, size_t np,
                                                     uint32_t* __restrict__ a2, uint32_t* __restrict__ b2) {
  typedef SnC C;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= np) return;
  const Fp<C> x = ld_fp<C>(ch), xi = ld_fp<C>(ch + 8);
  st_raw<C>(a2 + i * 8, fp_add(fp_mul(x, ld_raw<C>(a + i * 8)), fp_mul(xi, ld_raw<C>(a + (np + i) * 8))));
  st_raw<C>(b2 + i * 8, fp_add(fp_mul(xi, ld_raw<C>(b + i * 8)), fp_mul(x, ld_raw<C>(b + (np + i) * 8))));
}
// the remaining levels (n <= 2048) in ONE block: AL / BL hold every level's vector, level j at offset off(j) = 2N - 2N/2^j elements
__global__ void __launch_bounds__(1024) k_ipa_fold_tail(uint32_t* __restrict__ AL, uint32_t* __restrict__ BL, const uint32_t* __restrict__ ch, size_t N, int lv0, int levels) {
  typedef SnC C;
  for (int j = lv0; j < levels; ++j) {
    const size_t n = N >> j, np = n / 2, o = 2 * N - ((2 * N) >> j), o2 = 2 * N - ((2 * N) >> (j + 1));
    const Fp<C> x = ld_fp<C>(ch + j * 32), xi = ld_fp<C>(ch + j * 32 + 8);
    for (size_t i = threadIdx.x; i < np; i += 1024) {
      st_raw<C>(AL + (o2 + i) * 8, fp_add(fp_mul(x, ld_raw<C>(AL + (o + i) * 8)), fp_mul(xi, ld_raw<C>(AL + (o + np + i) * 8))));
      st_raw<C>(BL + (o2 + i) * 8, fp_add(fp_mul(xi, ld_raw<C>(BL + (o + i) * 8)), fp_mul(x, ld_raw<C>(BL + (o + np + i) * 8))));
    }
    __syncthreads();
  }
}
// scalars of the single MSM for the generators gg[k] and hh[k]: sF minus the levels' sum, all levels walked with wG[k], wH[k] in registers
__global__ void __launch_bounds__(256) k_ipa_verdict_scalars(const uint32_t* __restrict__ AL, const uint32_t* __restrict__ BL, const uint32_t* __restrict__ ch,
                                                             const uint32_t* __restrict__ wH0, size_t N, int levels, uint32_t* __restrict__ sF) {
  typedef SnC C;
  // the 4 * levels challenge values in Montgomery form, converted ONCE per block (every thread used to convert all of them itself: a third of this kernel's multiplications)
  __shared__ uint32_t chm[4 * 32 * C::N];
  for (int q = threadIdx.x; q < 4 * levels && q < 4 * 32; q += 256) st_raw<C>(chm + q * C::N, ld_fp<C>(ch + q * 8));
  __syncthreads();
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k >= N) return;
  Fp<C> wg = fp_one<C>(), wh = wH0 ? ld_fp<C>(wH0 + k * 8) : fp_one<C>();              // Montgomery form in registers
  Fp<C> cg = fp_zero<C>(), chh = fp_zero<C>();
  for (int j = 0; j < levels; ++j) {
    const size_t n = N >> j, np = n / 2, o = 2 * N - ((2 * N) >> j), i = k & (n - 1);
    const bool hi = i >= np; const size_t idx = hi ? i - np : np + i;                      // k_ipa_level_scalars: a[(hi ? j : np + j)]
    const Fp<C> x = ld_raw<C>(chm + (j * 4 + 0) * C::N), xi = ld_raw<C>(chm + (j * 4 + 1) * C::N), x2 = ld_raw<C>(chm + (j * 4 + 2) * C::N), x2i = ld_raw<C>(chm + (j * 4 + 3) * C::N);
    const Fp<C> sg = fp_mul(ld_fp<C>(AL + (o + idx) * 8), wg), sh = fp_mul(ld_fp<C>(BL + (o + idx) * 8), wh);
    cg = fp_add(cg, fp_mul(hi ? x2 : x2i, sg));                                           // gg_hi * a_lo belongs to L (x^2), gg_lo * a_hi to R (x^-2)
    chh = fp_add(chh, fp_mul(hi ? x2i : x2, sh));                                         // hh_lo * b_hi belongs to L, hh_hi * b_lo to R
    wg = fp_mul(wg, hi ? x : xi); wh = fp_mul(wh, hi ? xi : x);                           // gg' = gg_lo x^-1 + gg_hi x, hh' = hh_lo x + hh_hi x^-1 (:44-45)
  }
  const size_t of = 2 * N - ((2 * N) >> levels);                                          // the final one-element vectors
  st_fp<C>(sF + k * 8, fp_sub(fp_mul(ld_fp<C>(AL + of * 8), wg), cg));
  st_fp<C>(sF + (N + k) * 8, fp_sub(fp_mul(ld_fp<C>(BL + of * 8), wh), chh));
}
// blocks (j, side, y): cL_j = <a_lo, b_hi> (side 0) or cR_j = <a_hi, b_lo> (side 1) of level j (:36-37), times x_j^2 / x_j^-2, as IPA_DOT_SPLIT partial sums
// part[(2j + side) * IPA_DOT_SPLIT + y] (Montgomery form).  (One block per (j, side) made the top level's 32,768 products a chain of 128 per thread: 0.44 ms of the
// argument's 2 ms on 32 of 256 CUs.)
static constexpr int IPA_DOT_SPLIT = 16;
__global__ void __launch_bounds__(256) k_ipa_u_dots(const uint32_t* __restrict__ AL, const uint32_t* __restrict__ BL, const uint32_t* __restrict__ ch, size_t N,
                                                    uint32_t* __restrict__ part) {
  typedef SnC C;
  __shared__ uint32_t lds[256 * C::N];
  const int j = blockIdx.x >> 1, side = blockIdx.x & 1, t = threadIdx.x;
  const size_t n = N >> j, np = n / 2, o = 2 * N - ((2 * N) >> j);
  const uint32_t* av = AL + (o + (side ? np : 0)) * 8; const uint32_t* bv = BL + (o + (side ? 0 : np)) * 8;
  Fp<C> acc = fp_zero<C>();
  for (size_t i = (size_t)blockIdx.y * 256 + t; i < np; i += (size_t)256 * IPA_DOT_SPLIT) acc = fp_add(acc, fp_mul(ld_fp<C>(av + i * 8), ld_fp<C>(bv + i * 8)));
  acc = block_sum_256<C>(lds, acc);
  if (t == 0) st_raw<C>(part + ((size_t)blockIdx.x * IPA_DOT_SPLIT + blockIdx.y) * 8, fp_mul(acc, ld_fp<C>(ch + j * 32 + (side ? 24 : 16))));
}
// sF[2N] = a_fin b_fin - sum of the parts (the coefficient of u)
__global__ void __launch_bounds__(64) k_ipa_u_scalar(const uint32_t* __restrict__ AL, const uint32_t* __restrict__ BL, const uint32_t* __restrict__ part, size_t N, int levels,
                                                     uint32_t* __restrict__ sF) {
  typedef SnC C;
  if (threadIdx.x || blockIdx.x) return;
  const size_t of = 2 * N - ((2 * N) >> levels);
  Fp<C> v = fp_mul(ld_fp<C>(AL + of * 8), ld_fp<C>(BL + of * 8));
  for (int i = 0; i < 2 * levels * IPA_DOT_SPLIT; ++i) v = fp_sub(v, ld_raw<C>(part + i * 8));
  st_fp<C>(sF + 2 * N * 8, v);
}

// dot = sum_i a[i]*b[i] (one block); PrimeFieldElems * PrimeFieldElems then sum (prime_field_elems.rs:90-174)
template <class C>
__global__ void __launch_bounds__(256) k_dot(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[256 * C::N];
  const int t = threadIdx.x;
  Fp<C> acc = fp_zero<C>();
  for (size_t i = t; i < n; i += 256) acc = fp_add(acc, fp_mul(ld_fp<C>(a + i * C::N), ld_raw<C>(b + i * C::N)));
  acc = block_sum_256<C>(lds, acc);
  if (t == 0) st_raw<C>(out, acc);
}
// out[i] = a[i]*s0 + b[i]*s1 (a' = a_lo x + a_hi x^-1, bulletproofs.rs:49-50)
template <class C>
__global__ void __launch_bounds__(256) k_fold(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ s0,
                                              const uint32_t* __restrict__ s1, size_t n, uint32_t* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fp<C> r = fp_add(fp_mul(ld_fp<C>(s0), ld_raw<C>(a + i * C::N)), fp_mul(ld_fp<C>(s1), ld_raw<C>(b + i * C::N)));
  st_raw<C>(out + i * C::N, r);
}

// ---- the range proof's vector algebra in ONE launch (bulletproofs.rs:72-127) -------------------------------------------------------
// Every challenge is the caller's (injected), so nothing a lane computes for index i waits for anything but the proof's scalars:
//   aR = aL - 1, l0 = aL - z, aRz = aR + z, r0 = y^i aRz + z^2 2^i, r1 = y^i sR, l = l0 + sL x, r = y^i (aRz + sR x) + z^2 2^i
// and the scalar vectors of the five generator sums go straight into the MSM slots' buffers ([gg part | hh part], zkt_bp_ipa_ctx::dsc):
//   slot 0: aL | aR      slot 1: sL | sR      slot 2: -z | (z y^i + z^2 2^i) y^-i      slot 3: sL x | sR x      slot 4 (no argument): l | r y^-i
// The seven sums the scalar stage needs — t0 = <l0,r0>, t1 = <sL,r0> + <l0,r1>, t2 = <sL,r1>, <l,r>, v = <aL,2^n>, sum y^i, sum 2^i — leave as
// per-block parts (k_rp_sums folds them), instead of one launch per vector operation (~50 us each, ~40 of them).
struct RpScalars { const uint32_t *y, *yinv, *z, *z2, *x; };
struct RpOut { uint32_t *s0, *s1, *s2, *s3, *s4, *l, *r, *yinv_n, *parts; };
template <class C>
__global__ void __launch_bounds__(256) k_rp_fused(const uint32_t* __restrict__ aL, const uint32_t* __restrict__ sL, const uint32_t* __restrict__ sR, RpScalars k, size_t n, RpOut o) {
  static_assert(C::W == 32, "canonical 32-bit-limb scalar field");
  __shared__ uint32_t lds[256 * C::N];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * 256 + t;
  const bool live = i < n;
  Fp<C> r2, one_raw = fp_zero<C>(); one_raw.v[0] = 1;
  for (int j = 0; j < C::N; ++j) r2.v[j] = C::r2(j);
  auto M = [&](const uint32_t* p) { return fp_mul(fp_canon32(ld_raw<C>(p)), r2); };       // canonical words -> Montgomery
  auto out = [&](uint32_t* p, const Fp<C>& v) { st_raw<C>(p, fp_mul(v, one_raw)); };        // Montgomery -> canonical words
  auto pw = [&](Fp<C> b, size_t e) { Fp<C> r = fp_one<C>(); for (; e; e >>= 1) { if (e & 1) r = fp_mul(r, b); b = fp_sqr(b); } return r; };
  const Fp<C> y = M(k.y), yinv = M(k.yinv), z = M(k.z), z2 = M(k.z2), x = M(k.x), one = fp_one<C>();
  Fp<C> sums[7];
  for (int q = 0; q < 7; ++q) sums[q] = fp_zero<C>();
  if (live) {
    const Fp<C> a = M(aL + i * C::N), sl = M(sL + i * C::N), sr = M(sR + i * C::N);
    const Fp<C> yi = pw(y, i), yni = pw(yinv, i), twi = pw(fp_add(one, one), i);
    const Fp<C> aR = fp_sub(a, one), l0 = fp_sub(a, z), aRz = fp_add(aR, z), z2two = fp_mul(z2, twi);
    const Fp<C> r0 = fp_add(fp_mul(yi, aRz), z2two), r1 = fp_mul(yi, sr);
    const Fp<C> slx = fp_mul(sl, x), srx = fp_mul(sr, x);
    const Fp<C> l = fp_add(l0, slx), r = fp_add(fp_mul(yi, fp_add(aRz, srx)), z2two);
    sums[0] = fp_mul(l0, r0); sums[1] = fp_add(fp_mul(sl, r0), fp_mul(l0, r1)); sums[2] = fp_mul(sl, r1); sums[3] = fp_mul(l, r);
    sums[4] = fp_mul(a, twi); sums[5] = yi; sums[6] = twi;
    const size_t w = C::N;
    out(o.s0 + i * w, a); out(o.s0 + (n + i) * w, aR);
    out(o.s1 + i * w, sl); out(o.s1 + (n + i) * w, sr);
    out(o.s2 + i * w, fp_neg(z)); out(o.s2 + (n + i) * w, fp_mul(fp_add(fp_mul(z, yi), z2two), yni));
    out(o.s3 + i * w, slx); out(o.s3 + (n + i) * w, srx);
    if (o.s4) { out(o.s4 + i * w, l); out(o.s4 + (n + i) * w, fp_mul(r, yni)); }
    out(o.l + i * w, l); out(o.r + i * w, r); out(o.yinv_n + i * w, yni);
  }
  if (i == 0) for (int q = 0; q < C::N; ++q) {                       // the scalar of the u entry (index 2n) of every slot: 0
    o.s0[2 * n * C::N + q] = 0; o.s1[2 * n * C::N + q] = 0; o.s2[2 * n * C::N + q] = 0; o.s3[2 * n * C::N + q] = 0; if (o.s4) o.s4[2 * n * C::N + q] = 0;
  }
  for (int q = 0; q < 7; ++q) {                                        // block sums, one after the other through the same 8 KB
    const Fp<C> sum = block_sum_256<C>(lds, sums[q]);
    if (t == 0) st_raw<C>(o.parts + ((size_t)q * gridDim.x + blockIdx.x) * C::N, sum);     // still in the Montgomery domain: k_rp_sums leaves it
  }
}
// sums[q] = sum over the blocks of parts[q][*], out of the Montgomery domain (7 canonical scalars, 8 words apart)
template <class C>
__global__ void __launch_bounds__(256) k_rp_sums(const uint32_t* __restrict__ parts, size_t nblk, uint32_t* __restrict__ sums) {
  __shared__ uint32_t lds[256 * C::N];
  const int t = threadIdx.x, q = blockIdx.x;
  Fp<C> acc = fp_zero<C>(), one_raw = fp_zero<C>(); one_raw.v[0] = 1;
  for (size_t b = t; b < nblk; b += 256) acc = fp_add(acc, ld_raw<C>(parts + ((size_t)q * nblk + b) * C::N));
  acc = block_sum_256<C>(lds, acc);
  if (t == 0) st_raw<C>(sums + (size_t)q * C::N, fp_mul(acc, one_raw));
}
}  // namespace zkt

using namespace zkt;

// Bulletproofs::inner_product_argument (bulletproofs.rs:19-55); xs = one injected challenge per level (log2 n of them).
// out_trace (optional, host): per level L, R and the folded P' (3 zkt_secp_affine) for level-by-level parity.
// Runs on the original generators (see k_ipa_level_scalars): one resident base set [gg | hh | u], two MSMs per level and one for the base case.
// The reference draws x independently of L and R (:42), so a level's scalar algebra does not wait for its MSMs: the scalar stage runs ahead on
// the caller's stream and up to IPA_SLOTS MSMs are in flight; for a trace, L x^2 and R x^-2 (:47) are multiplied on side streams as results arrive.
// The generators are the long-lived input (one set per deployment): zkt_bp_ipa_ctx keeps their window-multiple table and every work buffer
// resident, and zkt_bp_inner_product_argument (the reference's signature) is create + run + free.
struct zkt_bp_ipa_ctx {
  static constexpr int IPA_SLOTS = 8;
  static constexpr size_t IPA_BATCH = 4;   // levels per product launch: a 256-bit double-and-add is ~4 ms however few points it covers
  size_t N, NB, levels, lv1;
  Dev dbase, da, db, da2, db2, dwG, dwH, dsc, dPp, dx, dch, dsq, dc, dlr, dm, dt;
  Dev dAL, dBL, dchall, dpart;             // verdict-only form: every level's a, b (2N elements each), all challenges, the u-entry parts
  zkt_secp_bases* set = nullptr;
  std::recursive_mutex mu;                 // a context serves one call at a time: concurrent callers queue here (the range proof re-enters for its inner-product argument)
  std::vector<hipStream_t> side;           // one stream per product batch, so the batches overlap each other and the MSMs
  hipEvent_t ev = nullptr, ev_null = nullptr;
  hipStream_t main = nullptr;              // the range proof's own stream: on the legacy NULL stream every one of its ~150 small launches pays the implicit barriers (~45 us each)
  // fixed-base tables (launch_fixed_table) of the range proof's g, h and of u: 3 x 64 points; g and h arrive per call and are cached by value
  Dev dfix{3 * 64 * SPB};
  // the range proof's work buffers (32 n-vectors, scalars, partial sums, points: range_proof_core carves them), kept with the context: seven hipMalloc and, worse, seven
  // hipFree per proof — each free waits for the whole device — were 0.26 ms of a 3.5 ms proof (hip trace, round 4)
  static constexpr int RP_NV = 32, RP_NS = 96;
  static size_t rp_arena_bytes(size_t n) { return (size_t)RP_NV * n * FRB + (size_t)RP_NS * FRB + 64 + 64 * FRB + 8 * 80 + 48 * 80 + 7 * ((n + 255) / 256) * FRB + 1024; }
  Dev rp_arena;
  zkt_secp_affine fix_g{}, fix_h{}; bool fix_g_ok = false, fix_h_ok = false, fix_u_ok = false;
  static size_t log2z(size_t n) { size_t l = 0; for (size_t t = n; t > 1; t >>= 1) ++l; return l; }
  explicit zkt_bp_ipa_ctx(size_t n)
      : N(n), NB(2 * n + 1), levels(log2z(n)), lv1(levels ? levels : 1), dbase(NB * SPB), da(N * FRB), db(N * FRB), da2(N * FRB), db2(N * FRB), dwG(N * FRB), dwH(N * FRB),
        dsc((size_t)IPA_SLOTS * NB * FRB), dPp(SPB), dx(lv1 * FRB), dch(2 * FRB), dsq(lv1 * 2 * FRB), dc(2 * FRB), dlr(lv1 * 2 * SPB), dm(lv1 * 2 * SPB), dt(SPB),
        dAL(2 * N * FRB), dBL(2 * N * FRB), dchall(lv1 * 4 * FRB), dpart(lv1 * 2 * 16 * FRB), rp_arena(rp_arena_bytes(n)) {}      // dpart: IPA_DOT_SPLIT (16) partial sums per (level, side)
  bool ok() const { return dfix.p && dbase.p && da.p && db.p && da2.p && db2.p && dwG.p && dwH.p && dsc.p && dPp.p && dx.p && dch.p && dsq.p && dc.p && dlr.p && dm.p && dt.p && dAL.p && dBL.p && dchall.p && dpart.p && rp_arena.p; }
  ~zkt_bp_ipa_ctx() {
    for (hipStream_t x : side) if (x) { hipStreamSynchronize(x); hipStreamDestroy(x); }
    if (main) { hipStreamSynchronize(main); hipStreamDestroy(main); }
    if (ev) hipEventDestroy(ev);
    if (ev_null) hipEventDestroy(ev_null);
    if (set) zkt_secp_bases_free(set);
  }
};

namespace {
constexpr int PW = 18; static_assert(PW * 4 == SPB, "zkt_secp_affine");      // u32 words of a secp256k1 point in the ABI layout
// The reference's one-shot calls (inner_product_argument, range_proof: bulletproofs.rs:19-55, 58-147) take the generators every time; a caller proves
// many statements over ONE generator set.  The last context built by a one-shot call (window-multiple table of 2n+1 points, work buffers, fixed-base
// tables: ~20 ms to set up at 65,536 generators) is kept and reused when the next call brings the same generators, byte for byte (host pointers only;
// zkt_shutdown releases it).
struct BpCtxCache { std::mutex mu; std::vector<uint8_t> key; std::shared_ptr<zkt_bp_ipa_ctx> ctx; } g_bpc;
bool bp_host_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return true; }      // unregistered host memory
  return a.type != hipMemoryTypeDevice;
}
std::shared_ptr<zkt_bp_ipa_ctx> bp_ctx_for(size_t n, const zkt_secp_affine* gg, const zkt_secp_affine* hh, const zkt_secp_affine* u, int* rc) {
  const bool cacheable = bp_host_ptr(gg) && bp_host_ptr(hh) && bp_host_ptr(u);
  const size_t nb = n * SPB;
  std::unique_lock<std::mutex> lk(g_bpc.mu, std::defer_lock);
  if (cacheable) {
    lk.lock();
    if (g_bpc.ctx && g_bpc.ctx->N == n && g_bpc.key.size() == 2 * nb + SPB && memcmp(g_bpc.key.data(), gg, nb) == 0 && memcmp(g_bpc.key.data() + nb, hh, nb) == 0 &&
        memcmp(g_bpc.key.data() + 2 * nb, u, SPB) == 0) { *rc = ZKT_OK; return g_bpc.ctx; }
  }
  zkt_bp_ipa_ctx* c = nullptr;
  *rc = zkt_bp_ipa_ctx_create(n, gg, hh, u, &c);
  if (*rc) return nullptr;
  std::shared_ptr<zkt_bp_ipa_ctx> sp(c, [](zkt_bp_ipa_ctx* q) { zkt_bp_ipa_ctx_free(q); });
  if (cacheable) {
    g_bpc.key.resize(2 * nb + SPB);
    memcpy(g_bpc.key.data(), gg, nb); memcpy(g_bpc.key.data() + nb, hh, nb); memcpy(g_bpc.key.data() + 2 * nb, u, SPB);
    g_bpc.ctx = sp;
  }
  return sp;
}

// The verdict-only argument in two halves, so that a caller can have it run beside its own work (the range proof does: everything up to the
// MSM needs a, b and the challenges only — P enters at the very end).  submit: scalar stage + the one MSM on `slot` (scalars in that slot's buffer);
// finish: collect, compare with P (host or device pointer).  Challenges must be invertible (checked by the callers).
int ipa_verdict_submit(zkt_bp_ipa_ctx* c, const uint64_t* a, const uint64_t* b, const uint64_t* xs, const uint32_t* wH0, hipStream_t s, int slot) {
  const size_t N = c->N, NB = c->NB, levels = c->levels;
  uint32_t *AL = c->dAL.w(), *BL = c->dBL.w(), *CH = c->dchall.w();
  if (hipMemcpyAsync(AL, a, N * FRB, hipMemcpyDefault, s) != hipSuccess || hipMemcpyAsync(BL, b, N * FRB, hipMemcpyDefault, s) != hipSuccess) return ZKT_ERR_DEVICE;
  int rc2;
  if ((rc2 = up(c->dx, xs, levels * FRB, s))) return rc2;
  hipLaunchKernelGGL(k_ipa_challenges_all, dim3(grid_blocks(levels, 64)), dim3(64), 0, s, (const uint32_t*)c->dx.w(), (int)levels, CH);
  size_t lv = 0;
  for (; lv < levels && (N >> lv) > 2048; ++lv) {
    const size_t np = (N >> lv) / 2, o = 2 * N - ((2 * N) >> lv), o2 = 2 * N - ((2 * N) >> (lv + 1));
    hipLaunchKernelGGL(k_ipa_fold_ab, dim3(grid_blocks(np)), dim3(256), 0, s, (const uint32_t*)(AL + o * 8), (const uint32_t*)(BL + o * 8), (const uint32_t*)(CH + lv * 32), np,
                       AL + o2 * 8, BL + o2 * 8);
  }
  if (lv < levels) hipLaunchKernelGGL(k_ipa_fold_tail, dim3(1), dim3(1024), 0, s, AL, BL, (const uint32_t*)CH, N, (int)lv, (int)levels);
  uint32_t* sF = c->dsc.w() + (size_t)slot * NB * 8;            // the slot's scalar buffer
  hipLaunchKernelGGL(k_ipa_verdict_scalars, dim3(grid_blocks(N)), dim3(256), 0, s, (const uint32_t*)AL, (const uint32_t*)BL, (const uint32_t*)CH, wH0, N, (int)levels, sF);
  hipLaunchKernelGGL(k_ipa_u_dots, dim3((unsigned)(2 * levels), IPA_DOT_SPLIT), dim3(256), 0, s, (const uint32_t*)AL, (const uint32_t*)BL, (const uint32_t*)CH, N, c->dpart.w());
  hipLaunchKernelGGL(k_ipa_u_scalar, dim3(1), dim3(64), 0, s, (const uint32_t*)AL, (const uint32_t*)BL, (const uint32_t*)c->dpart.w(), N, (int)levels, sF);
  if (hipGetLastError() != hipSuccess) return ZKT_ERR_DEVICE;
  return zkt_secp_msm_submit(c->set, (const uint64_t*)sF, NB, s, slot);
}
int ipa_verdict_finish(zkt_bp_ipa_ctx* c, int slot, const zkt_secp_affine* P, hipStream_t s) {      // 1 / 0, negative = -status
  zkt_secp_affine rhs, lhs;
  int rc2;
  if ((rc2 = zkt_secp_msm_collect(c->set, slot, &rhs, nullptr))) return -rc2;
  if (hipMemcpyAsync(&lhs, P, SPB, hipMemcpyDefault, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -ZKT_ERR_DEVICE;
  return memcmp(&rhs, &lhs, SPB) == 0 ? 1 : 0;
}
// one argument over the context's generators; a context serves one call at a time.  Returns 1 / 0 like the reference's bool, negative = -status.
int ipa_run(zkt_bp_ipa_ctx* c, const zkt_secp_affine* P, const uint64_t* a, const uint64_t* b, const uint64_t* xs, zkt_secp_affine* out_trace, const uint32_t* wH0) {
  if (zkt_internal_ready() != ZKT_OK) return -ZKT_ERR_DEVICE;
  if (!c || !P || !a || !b || (c->N > 1 && !xs)) return -ZKT_ERR_SHAPE;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  hipStream_t s = nullptr;
  constexpr int IPA_SLOTS = zkt_bp_ipa_ctx::IPA_SLOTS;
  constexpr size_t IPA_BATCH = zkt_bp_ipa_ctx::IPA_BATCH;
  const size_t N = c->N, NB = c->NB, levels = c->levels;
  size_t n = N;
  for (size_t lv = 0; lv < levels; ++lv) {                    // challenge x (:42, injected) must be invertible
    bool zero = true; for (int j = 0; j < 4; ++j) zero = zero && xs[lv * 4 + j] == 0;
    if (zero) return -ZKT_ERR_INV_ZERO;
  }
  if (!out_trace && levels >= 1) {           // verdict only: one MSM (see k_ipa_challenges_all)
    int rc2 = ipa_verdict_submit(c, a, b, xs, wH0, s, 0);
    if (rc2) return -rc2;
    return ipa_verdict_finish(c, 0, P, s);
  }
  // a trace was asked for, or n = 1 (no level: the base case alone): the level-by-level form
  Dev &da = c->da, &db = c->db, &da2 = c->da2, &db2 = c->db2, &dwG = c->dwG, &dwH = c->dwH, &dsc = c->dsc, &dPp = c->dPp, &dx = c->dx, &dch = c->dch, &dsq = c->dsq, &dc = c->dc,
      &dlr = c->dlr, &dm = c->dm, &dt = c->dt;
  int rc;
  if (hipMemcpyAsync(da.p, a, N * FRB, hipMemcpyDefault, s) != hipSuccess || hipMemcpyAsync(db.p, b, N * FRB, hipMemcpyDefault, s) != hipSuccess ||
      hipMemcpyAsync(dPp.p, P, SPB, hipMemcpyDefault, s) != hipSuccess) return -ZKT_ERR_DEVICE;                                  // P, a, b: host or device
  if ((rc = up(dx, xs, levels * FRB, s))) return -rc;
  const unsigned gN = grid_blocks(N + 1);                      // N + 1 threads
  hipLaunchKernelGGL(k_ipa_w_init, dim3(gN), dim3(256), 0, s, N, wH0, dwG.w(), dwH.w());
  uint32_t *Av = da.w(), *Bv = db.w(), *A2 = da2.w(), *B2 = db2.w();
  std::vector<zkt_secp_affine> lr(2 * levels + 1);            // L_0, R_0, L_1, R_1, ..., base-case right-hand side
  const size_t n_msm = 2 * levels + 1;
  size_t collected = 0, submitted = 0;
  struct Drain { zkt_bp_ipa_ctx* c; size_t *col, *sub; ~Drain() { for (; *col < *sub; ++*col) zkt_secp_msm_collect(c->set, (int)(*col % zkt_bp_ipa_ctx::IPA_SLOTS), nullptr, nullptr); } } drain{c, &collected, &submitted};
  // MSM m uses slot m % IPA_SLOTS and that slot's scalar buffer; results are collected in order, and once IPA_BATCH levels are in, their products start
  auto collect_next = [&]() -> int {
    const size_t m = collected;
    int r = zkt_secp_msm_collect(c->set, (int)(m % IPA_SLOTS), &lr[m], nullptr);
    ++collected;
    if (r) return r;
    if (out_trace && m < 2 * levels && (m & 1) && ((m / 2 + 1) % IPA_BATCH == 0 || m / 2 + 1 == levels)) {
      const size_t lv = m / 2, lv0 = lv / IPA_BATCH * IPA_BATCH, cnt = 2 * (lv + 1 - lv0);
      hipStream_t st = c->side[lv / IPA_BATCH];
      if (hipEventRecord(c->ev, s) != hipSuccess || hipStreamWaitEvent(st, c->ev, 0) != hipSuccess ||                   // x^2, x^-2 of these levels exist
          hipMemcpyAsync(dlr.w() + 2 * lv0 * PW, &lr[2 * lv0], cnt * SPB, hipMemcpyHostToDevice, st) != hipSuccess ||
          launch_group_mul(G_SECP, dlr.w() + 2 * lv0 * PW, dsq.w() + lv0 * 16, 8, dm.w() + 2 * lv0 * PW, cnt, st)) return ZKT_ERR_DEVICE;
    }
    return ZKT_OK;
  };
  auto slot_buf = [&](size_t m) -> uint32_t* { return dsc.w() + (m % IPA_SLOTS) * NB * 8; };
  auto free_slot = [&](size_t m) -> int { while (m >= collected + IPA_SLOTS) { int r = collect_next(); if (r) return r; } return ZKT_OK; };
  auto submit = [&](size_t m) -> int { int r = zkt_secp_msm_submit(c->set, (const uint64_t*)slot_buf(m), NB, s, (int)(m % IPA_SLOTS)); if (!r) ++submitted; return r; };
  size_t level = 0;
  while (n > 1) {
    const size_t np = n / 2, m = 2 * level;
    if ((rc = free_slot(m + 1))) return -rc;
    // cL = <a_lo, b_hi>, cR = <a_hi, b_lo>  (:36-37)
    hipLaunchKernelGGL(k_dot<SnC>, dim3(1), dim3(256), 0, s, (const uint32_t*)Av, (const uint32_t*)(Bv + np * 8), np, dc.w());
    hipLaunchKernelGGL(k_dot<SnC>, dim3(1), dim3(256), 0, s, (const uint32_t*)(Av + np * 8), (const uint32_t*)Bv, np, dc.w() + 8);
    // L = (gg_hi * a_lo).sum() + (hh_lo * b_hi).sum() + u * cL   (:39)
    // R = (gg_lo * a_hi).sum() + (hh_hi * b_lo).sum() + u * cR   (:40)
    hipLaunchKernelGGL(k_ipa_level_scalars, dim3(gN), dim3(256), 0, s, (const uint32_t*)Av, (const uint32_t*)Bv, (const uint32_t*)dwG.w(), (const uint32_t*)dwH.w(),
                       (const uint32_t*)dc.w(), N, n, slot_buf(m), slot_buf(m + 1));
    if (hipGetLastError() != hipSuccess) return -ZKT_ERR_DEVICE;
    if ((rc = submit(m)) || (rc = submit(m + 1))) return -rc;
    // x, x^-1, x^2, x^-2; generator coefficients and a' = a_lo x + a_hi x^-1 ; b' = b_lo x^-1 + b_hi x   (:44-45, :49-50)
    hipLaunchKernelGGL(k_ipa_challenge, dim3(1), dim3(64), 0, s, (const uint32_t*)(dx.w() + level * 8), dch.w(), dsq.w() + level * 16);
    const uint32_t *X = dch.w(), *XI = dch.w() + 8;
    hipLaunchKernelGGL(k_ipa_w_fold, dim3(gN), dim3(256), 0, s, X, XI, N, n, dwG.w(), dwH.w());
    hipLaunchKernelGGL(k_fold<SnC>, dim3(grid_blocks(np)), dim3(256), 0, s, (const uint32_t*)Av, (const uint32_t*)(Av + np * 8), X, XI, np, A2);
    hipLaunchKernelGGL(k_fold<SnC>, dim3(grid_blocks(np)), dim3(256), 0, s, (const uint32_t*)Bv, (const uint32_t*)(Bv + np * 8), XI, X, np, B2);
    std::swap(Av, A2); std::swap(Bv, B2);
    n = np; ++level;
  }
  // base case (:28-32): c = a*b; rhs = g*a + h*b + u*c over the original generators
  if ((rc = free_slot(n_msm - 1))) return -rc;
  hipLaunchKernelGGL(k_ipa_final_scalars, dim3(gN), dim3(256), 0, s, (const uint32_t*)Av, (const uint32_t*)Bv, (const uint32_t*)dwG.w(), (const uint32_t*)dwH.w(), N, slot_buf(n_msm - 1));
  if (hipGetLastError() != hipSuccess) return -ZKT_ERR_DEVICE;
  if ((rc = submit(n_msm - 1))) return -rc;
  while (collected < n_msm) if ((rc = collect_next())) return -rc;
  // P' = L x^2 + P + R x^-2 (:47) level by level for the trace (products ready on the side streams)
  if (out_trace) {
    for (hipStream_t x : c->side) if (hipStreamSynchronize(x) != hipSuccess) return -ZKT_ERR_DEVICE;
    for (size_t lv = 0; lv < levels; ++lv) {
      if (launch_group_add(G_SECP, dm.w() + 2 * lv * PW, dPp.w(), dt.w(), 1, s) || launch_group_add(G_SECP, dt.w(), dm.w() + (2 * lv + 1) * PW, dPp.w(), 1, s)) return -ZKT_ERR_DEVICE;
      out_trace[lv * 3] = lr[2 * lv]; out_trace[lv * 3 + 1] = lr[2 * lv + 1];
      if ((rc = down(out_trace + lv * 3 + 2, dPp.p, SPB, s))) return -rc;
    }
  }
  zkt_secp_affine lhs;
  if ((rc = down(&lhs, dPp.p, SPB, s))) return -rc;
  if (hipStreamSynchronize(s) != hipSuccess) return -ZKT_ERR_DEVICE;
  return memcmp(&lr[n_msm - 1], &lhs, SPB) == 0 ? 1 : 0;
}

// Bulletproofs::range_proof (bulletproofs.rs:58-147) over secp256k1, every random draw injected.
// rnd = alpha, rho, y, z, tau1, tau2, x, sL[n], sR[n] (4-limb residues mod the group order); u = the random point of :137;
// xs = IPA challenges.  out_pts (optional) = A, S, T1, T2, P.  Returns 1/0 like the reference's bool, negative = -status.
int range_proof_core(zkt_bp_ipa_ctx* c, const zkt_secp_affine* V, const uint64_t* aL, const uint64_t* gamma, const zkt_secp_affine* g, const zkt_secp_affine* h,
                     int use_ipa, const uint64_t* rnd, const uint64_t* xs, zkt_secp_affine* out_pts) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  const size_t n = c->N;
  hipStream_t s = c->main;
  // Order the proof's own (non-blocking) stream behind whatever was queued on the legacy NULL stream — the context's uploads and table build run there, and so
  // does the inner-product argument of the previous proof.  An event does that without waiting for anyone else's streams (a hipDeviceSynchronize() here stalled
  // every other thread's MSM pipelines once per proof).
  if (hipEventRecord(c->ev_null, nullptr) != hipSuccess || hipStreamWaitEvent(s, c->ev_null, 0) != hipSuccess) return -ZKT_ERR_DEVICE;
  // scalar-field vectors on the device (canonical residues), simple arena of n-vectors and scalars
  const int NV = zkt_bp_ipa_ctx::RP_NV, NS = zkt_bp_ipa_ctx::RP_NS;
  struct View { uint8_t* p; uint32_t* w() const { return (uint32_t*)p; } };                 // carved from the context's arena (the context's lock is held: one proof at a time)
  uint8_t* arena = (uint8_t*)c->rp_arena.p;
  auto carve = [&](size_t bytes) { View v{arena}; arena += (bytes + 63) & ~(size_t)63; return v; };
  static_assert(sizeof(zkt_secp_affine) <= 80, "arena sizing");
  const View vec = carve((size_t)NV * n * FRB), sc = carve((size_t)NS * FRB), derr = carve(8);
  unsigned long long* const noerr = (unsigned long long*)derr.p;
  int vi = 0, si = 0;
  auto newv = [&]() { return vec.w() + (size_t)(vi++) * n * 8; };
  auto news = [&]() { return sc.w() + (size_t)(si++) * 8; };
  // one-element operations are queued and run as ONE launch (launch_scalar_ops) when something is about to read their results: a launch per
  // operation is ~50 us of a chain of ~35
  ScalarOps pend{}; bool sok = true;
  auto sflush = [&]() { if (pend.n) { sok = sok && launch_scalar_ops(F_SN, pend, noerr, s) == hipSuccess; pend.n = 0; } };
  auto sop = [&](int o, const uint32_t* a, const uint32_t* b) { uint32_t* out = news(); if (pend.n == 48) sflush(); pend.o[pend.n++] = ScalarOp{o, a, b, out}; return out; };
  auto sadd = [&](const uint32_t* a, const uint32_t* b) { return sop(OP_ADD, a, b); };
  auto ssub = [&](const uint32_t* a, const uint32_t* b) { return sop(OP_SUB, a, b); };
  auto smul = [&](const uint32_t* a, const uint32_t* b) { return sop(OP_MUL, a, b); };
  auto sinv = [&](const uint32_t* a) { return sop(OP_INV, a, nullptr); };
  auto sput = [&](const uint64_t* hsrc) { uint32_t* o = news(); hipMemcpyAsync(o, hsrc, FRB, hipMemcpyHostToDevice, s); return o; };
  auto vput = [&](const uint64_t* hsrc) { uint32_t* o = newv(); hipMemcpyAsync(o, hsrc, n * FRB, hipMemcpyHostToDevice, s); return o; };
  unsigned long long ne = NO_ERR; hipMemcpyAsync(derr.p, &ne, 8, hipMemcpyHostToDevice, s);
  if ((rnd[8] | rnd[9] | rnd[10] | rnd[11]) == 0) return -ZKT_ERR_INV_ZERO;   // y must be invertible (:109); the reference draws non-zero values
  // The generators stay resident for the whole proof: one base set [gg | hh | u] (zkt_bp_ipa_ctx) serves every (AffinePoints * PrimeFieldElems).sum()
  // as an MSM and the inner-product argument itself.  hh' = hh * y^-i (:109) is never materialised: a sum over hh' with scalars v is the sum over hh
  // with scalars v o y^-n, and the argument starts from the coefficients y^-i on hh.  res = A S T1 T2 P | single-point scratch.
  int rc;
  const size_t NB = c->NB;
  const View pts = carve(8 * SPB), res = carve(48 * SPB);
  uint32_t *Gp = pts.w(), *Hp = Gp + PW, *Vp = Hp + PW, *Up = c->dbase.w() + 2 * n * PW;
  hipMemcpyAsync(Gp, g, SPB, hipMemcpyHostToDevice, s); hipMemcpyAsync(Hp, h, SPB, hipMemcpyHostToDevice, s); hipMemcpyAsync(Vp, V, SPB, hipMemcpyHostToDevice, s);
  uint32_t* R = res.w();
  uint32_t *Ak = R, *Sk = R + PW, *T1k = R + 2 * PW, *T2k = R + 3 * PW, *Pk = R + 4 * PW;        // out_pts order
  auto Q = [&](int i) { return R + (size_t)(8 + i) * PW; };                                       // single-point scratch
  // A scalar multiplication is a ~4-6 ms dependent chain however few points a launch covers, so the single-point multiplications go out in two
  // launches (everything independent of earlier POINTS first) while the MSMs run on the base set's streams.
  bool okl = true;
  auto seg = [&](const uint32_t* P, const uint32_t* k, uint32_t* out) { return MulSeg{P, k, out, 1u, 0u, 0u}; };
  auto run = [&](const MulSegs& m) { okl = okl && launch_group_mul_segs(G_SECP, m, 8, s) == hipSuccess; };
  auto padd = [&](const uint32_t* a, const uint32_t* b, uint32_t* o) { okl = okl && launch_group_add(G_SECP, a, b, o, 1, s) == hipSuccess; return o; };
  int n_sub = 0;
  zkt_secp_affine hres[5];
  int n_col = 0;
  bool ipa_started = false;                                                           // the inner-product argument's own MSM, in flight on IPA_SLOT beside the proof's
  constexpr int IPA_SLOT = 5;
  struct Drain { zkt_bp_ipa_ctx* c; int *col, *sub; bool* ipa; int ipa_slot;
    ~Drain() { for (; *col < *sub; ++*col) zkt_secp_msm_collect(c->set, *col, nullptr, nullptr); if (*ipa) zkt_secp_msm_collect(c->set, ipa_slot, nullptr, nullptr); } } drain{c, &n_col, &n_sub, &ipa_started, IPA_SLOT};
  auto msm_col = [&](int slot, uint32_t* dev_out) {                                               // slots are collected in order
    okl = okl && slot == n_col && zkt_secp_msm_collect(c->set, slot, &hres[slot], nullptr) == ZKT_OK; n_col = slot + 1;
    okl = okl && hipMemcpyAsync(dev_out, &hres[slot], SPB, hipMemcpyHostToDevice, s) == hipSuccess;
  };

  uint32_t *d_aL = vput(aL), *d_sL = vput(rnd + 28), *d_sR = vput(rnd + 28 + 4 * n);
  uint32_t *alpha = sput(rnd), *rho = sput(rnd + 4), *y = sput(rnd + 8), *z = sput(rnd + 12), *tau1 = sput(rnd + 16), *tau2 = sput(rnd + 20), *x = sput(rnd + 24);
  uint32_t* d_gamma = sput(gamma);
  const View dparts7 = carve(7 * ((n + 255) / 256) * FRB);
  // the whole vector stage in one launch (k_rp_fused)
  uint32_t* z2 = smul(z, z);
  uint32_t *yinv = sinv(y), *x2 = smul(x, x), *z3 = smul(z2, z);
  sflush();
  auto slot = [&](int k) { return c->dsc.w() + (size_t)k * NB * 8; };
  uint32_t *l = newv(), *r = newv(), *yinv_n = newv();
  uint32_t* sums = news(); for (int q = 1; q < 7; ++q) (void)news();                 // seven consecutive scalars
  const size_t nblk = grid_blocks(n);
  hipLaunchKernelGGL(k_rp_fused<SnC>, dim3((unsigned)nblk), dim3(256), 0, s, (const uint32_t*)d_aL, (const uint32_t*)d_sL, (const uint32_t*)d_sR,
                     RpScalars{y, yinv, z, z2, x}, n, RpOut{slot(0), slot(1), slot(2), slot(3), use_ipa ? nullptr : slot(4), l, r, yinv_n, dparts7.w()});
  hipLaunchKernelGGL(k_rp_sums<SnC>, dim3(7), dim3(256), 0, s, (const uint32_t*)dparts7.w(), nblk, sums);
  for (int k = 0; k < (use_ipa ? 4 : 5); ++k) { okl = okl && zkt_secp_msm_submit(c->set, (const uint64_t*)slot(k), NB, s, k) == ZKT_OK; if (okl) n_sub = k + 1; }
  // The argument's scalar stage and its one MSM need l, r and the challenges only — its P enters at the very end — so it starts NOW and runs beside the
  // proof's own generator sums.  The reference reaches it only after :116-118 hold; a proof that fails there is rejected below whatever the argument says,
  // and a zero challenge (its error) keeps the sequential order.
  if (use_ipa && c->levels >= 1 && xs) {
    bool nz = true;
    for (size_t lv = 0; lv < c->levels && nz; ++lv) nz = (xs[lv * 4] | xs[lv * 4 + 1] | xs[lv * 4 + 2] | xs[lv * 4 + 3]) != 0;
    if (nz && okl) { okl = ipa_verdict_submit(c, (const uint64_t*)l, (const uint64_t*)r, xs, yinv_n, s, IPA_SLOT) == ZKT_OK; ipa_started = okl; }      // (a side stream for its ~1 ms of small kernels measured no better: 6.5 against 6.2 ms)
  }
  uint32_t *t0 = sums, *t1 = sums + 8, *t2 = sums + 16, *lr = sums + 24, *v_val = sums + 32, *sum_y = sums + 5 * 8, *sum_2 = sums + 6 * 8;
  uint32_t* t_hat = sadd(sadd(t0, smul(t1, x)), smul(t2, x2));                      // :104
  uint32_t* tau_x = sadd(sadd(smul(tau2, x2), smul(tau1, x)), smul(z2, d_gamma));   // :105
  uint32_t* mu = sadd(alpha, smul(rho, x));                                         // :106
  uint32_t* delta_yz = ssub(smul(ssub(z, z2), sum_y), smul(z3, sum_2));             // :112
  // Every single-point product is a ~4 ms dependent chain however few points a launch covers, so ALL of them go out in ONE launch: the products the
  // reference takes of T1, T2 and S (:115, :124) are rewritten on the fixed points — T1 x = g (t1 x) + h (tau1 x), S x = h (rho x) + sum over the
  // generators with scalars sL x, sR x (one more MSM) — the same group elements, so A, S, T1, T2, P keep their bits.
  uint32_t* k_g = sadd(sadd(delta_yz, smul(t1, x)), smul(t2, x2));                  // rhs of :115 = V z^2 + g (delta + t1 x + t2 x^2) + h (tau1 x + tau2 x^2)
  uint32_t* k_h = sadd(smul(tau1, x), smul(tau2, x2));
  // ... and every one of them is on a FIXED point but one: g, h, u get 64-entry tables of their 16^w multiples (built when the context first sees
  // the point, ~4 ms once) and a product is one wave adding 64 partial products (~0.2 ms).  The exception is V z^2 (:115): V is the caller's.  For
  // the V this proof is about — V = g v + h gamma, v = <aL, 2^n> — it equals g (v z^2) + h (gamma z^2), which folds into the other two terms of
  // that side; E = g v + h gamma is computed beside and compared with V on the host, and any other V takes the 255-step product below.
  uint32_t *Tg = c->dfix.w(), *Th = Tg + 64 * PW, *Tu = Th + 64 * PW;
  auto same_point = [](const zkt_secp_affine& a, const zkt_secp_affine& b) { return memcmp(a.x, b.x, 32) == 0 && memcmp(a.y, b.y, 32) == 0 && a.is_infinity == b.is_infinity; };
  {
    FixedTables ft{}; int k = 0;
    const bool need_g = !c->fix_g_ok || !same_point(c->fix_g, *g), need_h = !c->fix_h_ok || !same_point(c->fix_h, *h), need_u = use_ipa && !c->fix_u_ok;
    if (need_g) { ft.point[k] = Gp; ft.table[k++] = Tg; }
    if (need_h) { ft.point[k] = Hp; ft.table[k++] = Th; }
    if (need_u) { ft.point[k] = Up; ft.table[k++] = Tu; }
    ft.n = k;
    okl = okl && launch_fixed_tables(G_SECP, ft, s) == hipSuccess;
    if (need_g) { c->fix_g = *g; c->fix_g_ok = okl; }
    if (need_h) { c->fix_h = *h; c->fix_h_ok = okl; }
    if (need_u) c->fix_u_ok = okl;
  }
  uint32_t *kg_v = sadd(k_g, smul(v_val, z2)), *kh_v = sadd(k_h, smul(d_gamma, z2));
  {
    FixedMuls m{}; int k = 0;
    auto fx = [&](const uint32_t* T, const uint32_t* kk, uint32_t* out) { m.m[k++] = FixedMul{T, kk, out}; };
    fx(Tg, t_hat, Q(8));   fx(Th, tau_x, Q(9));                                        // lhs of :116
    fx(Tg, kg_v, Q(11));   fx(Th, kh_v, Q(14));                                        // rhs of :115 with V z^2 folded in
    fx(Tg, v_val, Q(27));  fx(Th, d_gamma, Q(28));                                     // E = g v + h gamma, to be compared with V
    fx(Th, mu, Q(12));                                                                 // h mu = h alpha + x (h rho)
    if (use_ipa) fx(Tu, lr, Q(17));
    if (out_pts) {
      fx(Th, alpha, Q(0)); fx(Th, rho, Q(1));
      fx(Tg, t1, Q(4));    fx(Th, tau1, Q(5));  fx(Tg, t2, Q(6));  fx(Th, tau2, Q(7));
    }
    m.n = k;
    sflush();
    okl = okl && launch_fixed_muls(G_SECP, m, s) == hipSuccess;
  }
  msm_col(0, Q(2)); msm_col(1, Q(3)); msm_col(2, Q(22)); msm_col(3, Q(16));
  if (!use_ipa) msm_col(4, Q(25));
  {                                                                                   // every remaining sum of single points in ONE launch, one lane per sum
    PointSums ps{}; int k = 0;
    auto sum = [&](uint32_t* out, std::initializer_list<const uint32_t*> in) { int j = 0; for (const uint32_t* q : in) ps.in[k][j++] = q; ps.cnt[k] = j; ps.out[k++] = out; };
    sum(Q(13), {Q(8), Q(9)});                                                         // lhs of :116
    sum(Q(20), {Q(11), Q(14)});                                                       // rhs of :115 (for V = g v + h gamma)
    sum(Q(29), {Q(27), Q(28)});                                                       // E
    sum(Q(21), {Q(2), Q(16), Q(22)});                                                 // P h^-mu: the three generator sums of A, S x and :126-127
    sum(Pk, {Q(2), Q(16), Q(22), Q(12)});                                             // P (:124-128) = h mu + those
    if (use_ipa) sum(Q(24), {Q(2), Q(16), Q(22), Q(17)});                             // :138  P h^-mu u^<l,r>: the argument's P
    if (out_pts) {
      sum(Ak, {Q(0), Q(2)});                                                          // A (:77)
      sum(Sk, {Q(1), Q(3)});                                                          // S (:82)
      sum(T1k, {Q(4), Q(5)}); sum(T2k, {Q(6), Q(7)});                                 // T1 (:99), T2 (:100)
    }
    ps.n = k;
    okl = okl && launch_point_sums(G_SECP, ps, s) == hipSuccess;
  }
  zkt_secp_affine hl, hr, hE;
  if ((rc = down(&hl, Q(13), SPB, s)) || (rc = down(&hr, Q(20), SPB, s)) || (rc = down(&hE, Q(29), SPB, s))) return -rc;
  if (out_pts && (rc = down(out_pts, R, 5 * SPB, s))) return -rc;
  sflush();
  if (hipStreamSynchronize(s) != hipSuccess || !okl || !sok || vi > NV || si > NS) return -ZKT_ERR_DEVICE;
  if (!same_point(hE, *V)) {                                                          // some other V: its own product, as the reference takes it (:115)
    MulSegs mv{}; mv.s[0] = seg(Vp, z2, Q(10)); mv.n = 1; sflush(); run(mv);
    FixedMuls m{}; m.m[0] = FixedMul{Tg, k_g, Q(11)}; m.m[1] = FixedMul{Th, k_h, Q(14)}; m.n = 2;
    okl = okl && launch_fixed_muls(G_SECP, m, s) == hipSuccess;
    padd(padd(Q(10), Q(11), Q(18)), Q(14), Q(20));
    if ((rc = down(&hr, Q(20), SPB, s))) return -rc;
    if (hipStreamSynchronize(s) != hipSuccess || !okl) return -ZKT_ERR_DEVICE;
  }
  if (memcmp(&hl, &hr, SPB) != 0) return 0;                                           // :116-118
  if (use_ipa) {
    uint32_t* Pp = Q(24);                                                             // :138, summed with the others above
    if (!okl) return -ZKT_ERR_DEVICE;
    if (ipa_started) { ipa_started = false; return ipa_verdict_finish(c, IPA_SLOT, (const zkt_secp_affine*)Pp, s); }      // :139, already in flight
    if (hipStreamSynchronize(s) != hipSuccess) return -ZKT_ERR_DEVICE;                // the argument runs on the NULL stream, which does not wait for a non-blocking one
    return ipa_run(c, (const zkt_secp_affine*)Pp, (const uint64_t*)l, (const uint64_t*)r, xs, nullptr, yinv_n);   // :139, over gg, hh' = y^-i hh, u
  }
  uint32_t* rhs = padd(Q(12), Q(25), Q(26));                                          // :142
  zkt_secp_affine hP, hrhs; uint64_t hth[4], hlr[4];
  if ((rc = down(&hP, Pk, SPB, s)) || (rc = down(&hrhs, rhs, SPB, s)) || (rc = down(hth, t_hat, FRB, s)) || (rc = down(hlr, lr, FRB, s))) return -rc;
  if (hipStreamSynchronize(s) != hipSuccess || !okl) return -ZKT_ERR_DEVICE;
  if (memcmp(&hP, &hrhs, SPB) != 0) return 0;
  return memcmp(hth, hlr, FRB) == 0 ? 1 : 0;                                          // :147-149
}
}  // namespace

extern "C" {
void bp_clear_caches() { std::lock_guard<std::mutex> lk(g_bpc.mu); g_bpc.ctx.reset(); g_bpc.key.clear(); }      // zkt_shutdown: the context kept for the one-shot calls
int zkt_bp_ipa_ctx_create(size_t n, const zkt_secp_affine* gg, const zkt_secp_affine* hh, const zkt_secp_affine* u, zkt_bp_ipa_ctx** out) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (n == 0 || (n & (n - 1)) || n > (size_t(1) << 24) || !gg || !hh || !u || !out) return ZKT_ERR_SHAPE;
  hipStream_t s = nullptr;
  std::unique_ptr<zkt_bp_ipa_ctx> c(new zkt_bp_ipa_ctx(n));
  if (!c->ok()) return ZKT_ERR_DEVICE;
  const size_t N = n;
  HIPCHK(hipMemcpyAsync(c->dbase.p, gg, N * SPB, hipMemcpyDefault, s));                        // host or device pointers (the range proof hands over hh' in HBM)
  HIPCHK(hipMemcpyAsync((char*)c->dbase.p + N * SPB, hh, N * SPB, hipMemcpyDefault, s));
  HIPCHK(hipMemcpyAsync((char*)c->dbase.p + 2 * N * SPB, u, SPB, hipMemcpyDefault, s));
  c->side.assign((c->levels + zkt_bp_ipa_ctx::IPA_BATCH - 1) / zkt_bp_ipa_ctx::IPA_BATCH, nullptr);
  for (hipStream_t& x : c->side) HIPCHK(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->ev, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_null, hipEventDisableTiming));
  HIPCHK(hipStreamCreateWithFlags(&c->main, hipStreamNonBlocking));
  int rc = zkt_secp_bases_from_device((const zkt_secp_affine*)c->dbase.p, c->NB, s, &c->set);
  if (rc) return rc;
  *out = c.release();
  return ZKT_OK;
}
void zkt_bp_ipa_ctx_free(zkt_bp_ipa_ctx* c) { delete c; }

int zkt_bp_inner_product_argument_ctx(zkt_bp_ipa_ctx* c, const zkt_secp_affine* P, const uint64_t* a, const uint64_t* b, const uint64_t* xs, zkt_secp_affine* out_trace) {
  return ipa_run(c, P, a, b, xs, out_trace, nullptr);
}
int zkt_bp_inner_product_argument(size_t n, const zkt_secp_affine* gg, const zkt_secp_affine* hh, const zkt_secp_affine* u, const zkt_secp_affine* P,
                                  const uint64_t* a, const uint64_t* b, const uint64_t* xs, zkt_secp_affine* out_trace) {
  if (n == 0 || (n & (n - 1)) || !gg || !hh || !u || !P || !a || !b || (n > 1 && !xs)) return -ZKT_ERR_SHAPE;
  int rc;
  const std::shared_ptr<zkt_bp_ipa_ctx> c = bp_ctx_for(n, gg, hh, u, &rc);
  if (rc) return -rc;
  return zkt_bp_inner_product_argument_ctx(c.get(), P, a, b, xs, out_trace);
}

int zkt_bp_range_proof(size_t n, const zkt_secp_affine* V, const uint64_t* aL, const uint64_t* gamma, const zkt_secp_affine* g, const zkt_secp_affine* h,
                       const zkt_secp_affine* gg, const zkt_secp_affine* hh, int use_ipa, const uint64_t* rnd, const zkt_secp_affine* u, const uint64_t* xs,
                       zkt_secp_affine* out_pts) {
  if (zkt_internal_ready() != ZKT_OK) return -ZKT_ERR_DEVICE;
  if (n == 0 || (n & (n - 1)) || !V || !aL || !gamma || !g || !h || !gg || !hh || !rnd || (use_ipa && (!u || (n > 1 && !xs)))) return -ZKT_ERR_SHAPE;
  zkt_secp_affine inf_pt; memset(&inf_pt, 0, sizeof inf_pt); inf_pt.is_infinity = 1;
  int rc;
  const std::shared_ptr<zkt_bp_ipa_ctx> c = bp_ctx_for(n, gg, hh, use_ipa ? u : &inf_pt, &rc);
  if (rc) return -rc;
  return range_proof_core(c.get(), V, aL, gamma, g, h, use_ipa, rnd, xs, out_pts);
}
// the same proof over a context's resident generators gg, hh, u (zkt_bp_ipa_ctx_create): no table build, no generator upload per proof
int zkt_bp_range_proof_ctx(zkt_bp_ipa_ctx* c, const zkt_secp_affine* V, const uint64_t* aL, const uint64_t* gamma, const zkt_secp_affine* g, const zkt_secp_affine* h,
                           int use_ipa, const uint64_t* rnd, const uint64_t* xs, zkt_secp_affine* out_pts) {
  if (zkt_internal_ready() != ZKT_OK) return -ZKT_ERR_DEVICE;
  if (!c || !V || !aL || !gamma || !g || !h || !rnd || (use_ipa && c->N > 1 && !xs)) return -ZKT_ERR_SHAPE;
  return range_proof_core(c, V, aL, gamma, g, h, use_ipa, rnd, xs, out_pts);
}
}  // extern "C"
