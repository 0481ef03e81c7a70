// Dense polynomials over Fr: the reference's Polynomial::{multiply_by, divide_by, eval_at, eval_from_1_to_n} (field/polynomial.rs:173-262),
// QAP::build_t / build_p (qap/qap.rs:99-135) and the quotient h = p / t of Prover::new (groth16/zktoolkit_based/prover.rs:64-71, pinocchio/prover.rs:50-96).
//
// The reference multiplies schoolbook and divides by long division, O(n^2) field operations.  Quotient and remainder are unique, and Fr has 2-adicity 32, so
// the same coefficients come out of exact NTT arithmetic:
//   product     min(na, nb) <= POLY_DIRECT_MAX: one lane per output coefficient over the shorter operand (k_mul_direct).  Otherwise both operands are
//               transformed at N = 2^ceil(log2(na + nb - 1)) by the LDS-fused transform of zkt_fr_vec.hip, the pointwise product rides on the last
//               launch of the second forward transform (its `mulvec`), and the 1/N rides on the pass that stores the result.  a == b shares one transform.
//   division    L = na - nb + 1 quotient coefficients.  rev(q) = rev(a) / rev(b) mod x^L is a power series quotient.  L <= POLY_DIV_DIRECT_MAX: one block
//               runs the triangular recurrence (k_div_direct).  Otherwise g = 1 / rev(b) by Newton steps p -> 2p from g = 1 / b_lead: with f g = 1 + x^p e
//               mod x^2p the update is g -= x^p (e g mod x^p); both products are CYCLIC at N = 2p (the wrapped part of f g lands below x^p, where the value
//               is known), so a step is three forward and two inverse transforms of size 2p.  Then rev(q) = rev(a) g mod x^L.
//   remainder   a - q b has fewer than nb - 1 coefficients, so it is computed modulo x^N - 1 with N = 2^ceil(log2(nb - 1)): q, b and a are folded to N
//               coefficients first (k_fold), whatever L is — a short divisor under a long quotient costs transforms of the divisor's size, not the dividend's.
//   t           product tree over (x - i): levels whose children have at most POLY_DIRECT_MAX roots go through one batched direct kernel, the levels above
//               through batched transforms (the children are monic, so the product's leading 1 that wraps at N = 2 * roots is put back by hand).
//   evaluation  one lane per point (Horner) when there are many points; few points of a long polynomial: blocks of EVAL_CHUNK coefficients, EVAL_ITEMS per
//               lane, an LDS tree over the lanes' partial values, and a short Horner over the blocks.
// Buffers hold Montgomery values; canonical <-> Montgomery happens in the first and the last kernel that touches the caller's data.
// Twiddle tables are cached per transform size (built on first use under a lock, released by zkt_shutdown); everything else a call needs is
// stream-ordered scratch (hipMallocAsync / hipFreeAsync on the call's stream).
// profiles/poly_timing.md has the measurements behind the two thresholds (tools/diag/poly_timing.py makes them); tests/poly_model.py restates this plan.
#include <vector>
#include <mutex>
#include <cstring>
#include "fr_vec.h"
#include "zkt_internal.h"
#include "../../include/zkt.h"
#include "host_abi.h"
#include "fr_pool.h"
#include "qap_handle.h"

namespace zkt {
namespace {
typedef FrC C;

#ifdef ZKT_POLY_TIMING_DIRECT         // scratch libraries of tools/diag/poly_timing.py only (one path forced); the shipped library has no switch
static constexpr size_t POLY_DIRECT_MAX = ZKT_POLY_TIMING_DIRECT;
static constexpr size_t POLY_DIV_DIRECT_MAX = ZKT_POLY_TIMING_DIV;
#else
static constexpr size_t POLY_DIRECT_MAX = 64;          // shorter operand of a product up to which k_mul_direct is used
static constexpr size_t POLY_DIV_DIRECT_MAX = 64;      // quotient length up to which k_div_direct is used
#endif
static constexpr int POLY_MAX_LOG = 21;                // ZKT_POLY_MAX_LEN = 2^21
static constexpr int EVAL_ITEMS = 16, EVAL_TPB = 256, EVAL_CHUNK = EVAL_ITEMS * EVAL_TPB;
static constexpr size_t EVAL_SPLIT_MIN_N = 2 * (size_t)EVAL_CHUNK;      // the split kernels from two blocks' worth of coefficients on ...
static constexpr size_t EVAL_SPLIT_MAX_K = 1024;                        // ... and below this many points (above it the points alone fill the device)
static_assert(((size_t)1 << POLY_MAX_LOG) == ZKT_POLY_MAX_LEN, "twiddle cache covers every transform size");

// dst[i] = src[start + step * i] (* *scale) for i < cnt, zero for cnt <= i < n: load, store, reversal, zero padding and the 1/N of a transform in one pass
template <bool IN_CANON, bool OUT_CANON>
__global__ void __launch_bounds__(256) k_gather(uint32_t* __restrict__ dst, size_t n, const uint32_t* __restrict__ src, size_t cnt, long long start, int step,
                                                const uint32_t* __restrict__ scale, int scale_sq) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  Fr v = fp_zero<C>();
  if (i < cnt) {
    v = ldx<IN_CANON>(src + (size_t)(start + (long long)step * (long long)i) * FW);
    if (scale) { Fr s = ldm4(scale); if (scale_sq) s = fp_sqr(s); v = fp_mul(v, s); }
  }
  stx<OUT_CANON>(dst + i * FW, v);
}
// out[k] = sum_j s[j] l[k - j] for k < keep, s the shorter operand (ns <= nl).  CANON: both operands and the result in the caller's layout — the canonical
// integers are multiplied as they are (each product is a b / R), and ONE multiplication by R^2 on the way out turns the sum into the canonical result
template <bool CANON>
__global__ void __launch_bounds__(256) k_mul_direct(const uint32_t* __restrict__ sh, size_t ns, const uint32_t* __restrict__ lg, size_t nl, uint32_t* __restrict__ out, size_t keep) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; if (k >= keep) return;
  const size_t j0 = k + 1 > nl ? k + 1 - nl : 0, j1 = k < ns - 1 ? k : ns - 1;
  Fr acc = fp_zero<C>();
  for (size_t j = j0; j <= j1; ++j) {
    Fr a = ldm4(sh + j * FW), b = ldm4(lg + (k - j) * FW);
    if (CANON) { a = fp_canon32(a); b = fp_canon32(b); }
    acc = fp_add(acc, fp_mul(a, b));
  }
  stm4(out + k * FW, CANON ? to_mont(acc) : acc);
}
__global__ void __launch_bounds__(256) k_sqr_all(uint32_t* __restrict__ a, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  stm4(a + i * FW, fp_sqr(ldm4(a + i * FW)));
}
// out[i] = a[i] - b[i] (* *scale on b), i < n; out may be a
template <bool OUT_CANON>
__global__ void __launch_bounds__(256) k_sub(uint32_t* out, const uint32_t* a, const uint32_t* __restrict__ b, size_t n, const uint32_t* __restrict__ scale) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  Fr v = ldm4(b + i * FW); if (scale) v = fp_mul(v, ldm4(scale));
  stx<OUT_CANON>(out + i * FW, fp_sub(ldm4(a + i * FW), v));
}
// dst[i] += a[i] + b[i], i < n
__global__ void __launch_bounds__(256) k_add2(uint32_t* __restrict__ dst, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  stm4(dst + i * FW, fp_add(ldm4(dst + i * FW), fp_add(ldm4(a + i * FW), ldm4(b + i * FW))));
}
// *out = 1 / *in (one lane); a zero is reported through err
__global__ void k_inv1(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, unsigned long long* err, unsigned long long index) {
  if (threadIdx.x || blockIdx.x) return;
  const Fr v = ldm4(in);
  if (fp_is_zero(v)) { atomicMin(err, index); stm4(out, v); return; }
  stm4(out, fp_inv(v));
}
// Power series quotient by the triangular recurrence, one block: with ra = rev(a), f = rev(b) and rq = rev(q),
// rq[k] = (ra[k] - sum_{1 <= j <= k} f[j] rq[k - j]) / f[0].  q[L-1-k] carries the running value of rq[k]; step k fixes it and subtracts its multiples from the later ones.
__global__ void __launch_bounds__(256) k_div_direct(const uint32_t* __restrict__ a, size_t na, const uint32_t* __restrict__ b, size_t nb, uint32_t* q, size_t L,
                                                    const uint32_t* __restrict__ finv) {
  const size_t t = threadIdx.x;
  for (size_t k = t; k < L; k += 256) stm4(q + (L - 1 - k) * FW, ldm4(a + (na - 1 - k) * FW));
  __syncthreads();
  const Fr fi = ldm4(finv);
  for (size_t k = 0; k < L; ++k) {
    const Fr v = fp_mul(ldm4(q + (L - 1 - k) * FW), fi);
    __syncthreads();
    if (t == 0) stm4(q + (L - 1 - k) * FW, v);
    for (size_t i = k + 1 + t; i < L && i - k < nb; i += 256)
      stm4(q + (L - 1 - i) * FW, fp_sub(ldm4(q + (L - 1 - i) * FW), fp_mul(ldm4(b + (nb - 1 - (i - k)) * FW), v)));
    __syncthreads();
  }
}
// Newton update: g[p + i] = -E[i] / N^2, i < cnt (E carries the N of two unscaled inverse transforms)
__global__ void __launch_bounds__(256) k_newton_update(uint32_t* __restrict__ g_hi, const uint32_t* __restrict__ E, size_t cnt, const uint32_t* __restrict__ ninv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= cnt) return;
  const Fr s = fp_sqr(ldm4(ninv));
  stm4(g_hi + i * FW, fp_neg(fp_mul(ldm4(E + i * FW), s)));
}
// dst[i] = sum of src[j] over j = i mod N, j < n: the polynomial modulo x^N - 1
__global__ void __launch_bounds__(256) k_fold(uint32_t* __restrict__ dst, size_t N, const uint32_t* __restrict__ src, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= N) return;
  Fr acc = fp_zero<C>();
  for (size_t j = i; j < n; j += N) acc = fp_add(acc, ldm4(src + j * FW));
  stm4(dst + i * FW, acc);
}
// *top = max(*top, i + 1) over the non-zero a[i]
__global__ void __launch_bounds__(256) k_top_nonzero(const uint32_t* __restrict__ a, size_t n, unsigned long long* top) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  if (!fp_is_zero(ldm4(a + i * FW))) atomicMax(top, (unsigned long long)(i + 1));
}

// ---- product tree of t = prod_{i=1..n} (x - i) ---------------------------------------------------------------------------
// A level of span s holds ceil(n / s) nodes, node j = prod over the roots j s + 1 .. min((j+1) s, n), s + 1 slots each (zeros above its degree).
__device__ inline size_t tree_deg(size_t n, size_t s, size_t j) { const size_t lo = j * s; return lo >= n ? 0 : (n - lo < s ? n - lo : s); }
__global__ void __launch_bounds__(256) k_tree_leaves(uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  stm4(out + 2 * i * FW, fp_neg(fr_small((uint32_t)(i + 1)))); stm4(out + (2 * i + 1) * FW, fp_one<C>());
}
// one lane per (node, coefficient) of the level of span 2s
__global__ void __launch_bounds__(256) k_tree_direct(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t s, size_t n, size_t nodes) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * s + 1; if (i >= nodes * per) return;
  const size_t j = i / per, k = i % per, dl = tree_deg(n, s, 2 * j), dr = tree_deg(n, s, 2 * j + 1);
  const uint32_t* l = src + (2 * j) * (s + 1) * FW; const uint32_t* r = src + (2 * j + 1) * (s + 1) * FW;
  Fr acc = fp_zero<C>();
  if (dr == 0) { if (k <= dl) acc = ldm4(l + k * FW); }               // an only child (the right one would be the constant 1)
  else if (k <= dl + dr) {
    const size_t i0 = k > dr ? k - dr : 0, i1 = k < dl ? k : dl;
    for (size_t a = i0; a <= i1; ++a) acc = fp_add(acc, fp_mul(ldm4(l + a * FW), ldm4(r + (k - a) * FW)));
  }
  stm4(dst + i * FW, acc);
}
// X[j] = left child of node j, Y[j] = right child (or the constant 1), each zero-padded to N = 2s
__global__ void __launch_bounds__(256) k_tree_gather(const uint32_t* __restrict__ src, uint32_t* __restrict__ X, uint32_t* __restrict__ Y, size_t s, size_t n, size_t nodes) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, N = 2 * s; if (i >= nodes * N) return;
  const size_t j = i / N, k = i % N, dl = tree_deg(n, s, 2 * j), dr = tree_deg(n, s, 2 * j + 1);
  stm4(X + i * FW, k <= dl ? ldm4(src + ((2 * j) * (s + 1) + k) * FW) : fp_zero<C>());
  Fr y = fp_zero<C>();
  if (dr == 0) { if (k == 0) y = fp_one<C>(); } else if (k <= dr) y = ldm4(src + ((2 * j + 1) * (s + 1) + k) * FW);
  stm4(Y + i * FW, y);
}
// the cyclic products X (times N) -> the level of span 2s: the leading 1 is written, and taken off coefficient 0 where it wrapped (two full children)
__global__ void __launch_bounds__(256) k_tree_scatter(const uint32_t* __restrict__ X, uint32_t* __restrict__ dst, size_t s, size_t n, size_t nodes, const uint32_t* __restrict__ ninv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * s + 1, N = 2 * s; if (i >= nodes * per) return;
  const size_t j = i / per, k = i % per, d = tree_deg(n, s, 2 * j) + tree_deg(n, s, 2 * j + 1);
  Fr v = fp_zero<C>();
  if (k == d) v = fp_one<C>();
  else if (k < d) { v = fp_mul(ldm4(X + (j * N + k) * FW), ldm4(ninv)); if (k == 0 && d == N) v = fp_sub(v, fp_one<C>()); }
  stm4(dst + i * FW, v);
}

// ---- evaluation ----------------------------------------------------------------------------------------------------
// one lane per point: Horner over the Montgomery coefficients
__global__ void __launch_bounds__(256) k_eval_horner(const uint32_t* __restrict__ coef, size_t n, const uint32_t* __restrict__ xs, size_t k, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= k) return;
  const Fr x = ldx<true>(xs + i * FW);
  Fr acc = ldm4(coef + (n - 1) * FW);
  for (size_t j = n - 1; j-- > 0;) acc = fp_add(fp_mul(acc, x), ldm4(coef + j * FW));
  stx<true>(out + i * FW, acc);
}
// block (c, point): sum_{e < EVAL_CHUNK} coef[c EVAL_CHUNK + e] x^e.  A lane runs Horner over its EVAL_ITEMS coefficients, then a tree over the lanes:
// at distance d the upper partner's value is worth x^(EVAL_ITEMS d).  part[point * chunks + c], Montgomery.
__global__ void __launch_bounds__(EVAL_TPB) k_eval_split(const uint32_t* __restrict__ coef, size_t n, const uint32_t* __restrict__ xs, size_t chunks, uint32_t* __restrict__ part) {
  __shared__ uint32_t lds[EVAL_TPB * FW];
  const int t = threadIdx.x;
  const Fr x = ldx<true>(xs + (size_t)blockIdx.y * FW);
  const size_t base = (size_t)blockIdx.x * EVAL_CHUNK + (size_t)t * EVAL_ITEMS;
  Fr acc = fp_zero<C>();
  for (int e = EVAL_ITEMS - 1; e >= 0; --e) { acc = fp_mul(acc, x); if (base + e < n) acc = fp_add(acc, ldm4(coef + (base + e) * FW)); }
  Fr xp = x;
  for (int e = 1; e < EVAL_ITEMS; e <<= 1) xp = fp_sqr(xp);                 // x^EVAL_ITEMS
  stm4(lds + t * FW, acc); __syncthreads();
  for (int d = 1; d < EVAL_TPB; d <<= 1) {
    if ((t & (2 * d - 1)) == 0) { acc = fp_add(acc, fp_mul(ldm4(lds + (t + d) * FW), xp)); stm4(lds + t * FW, acc); }
    xp = fp_sqr(xp);
    __syncthreads();
  }
  if (t == 0) stm4(part + ((size_t)blockIdx.y * chunks + blockIdx.x) * FW, acc);
}
// one lane per point: Horner over its blocks in y = x^EVAL_CHUNK
__global__ void __launch_bounds__(256) k_eval_combine(const uint32_t* __restrict__ part, size_t chunks, const uint32_t* __restrict__ xs, size_t k, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= k) return;
  Fr y = ldx<true>(xs + i * FW);
  for (int e = 1; e < EVAL_CHUNK; e <<= 1) y = fp_sqr(y);
  const uint32_t* p = part + i * chunks * FW;
  Fr acc = ldm4(p + (chunks - 1) * FW);
  for (size_t j = chunks - 1; j-- > 0;) acc = fp_add(fp_mul(acc, y), ldm4(p + j * FW));
  stx<true>(out + i * FW, acc);
}
// out[p][j] = sum_i wires[i] M_p[i][j], p = blockIdx.y over the three rows x n coefficient arrays (caller's layout in, Montgomery out)
struct Comb3 { const uint32_t* m[3]; uint32_t* out[3]; };
__global__ void __launch_bounds__(256) k_wire_comb(Comb3 c, const uint32_t* __restrict__ wires, size_t rows, size_t n) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; if (j >= n) return;
  const uint32_t* m = c.m[blockIdx.y];
  Fr acc = fp_zero<C>();
  for (size_t i = 0; i < rows; ++i) acc = fp_add(acc, fp_mul(ldx<true>(wires + i * FW), ldx<true>(m + (i * n + j) * FW)));
  stm4(c.out[blockIdx.y] + j * FW, acc);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// twiddle tables per transform size, kept until zkt_shutdown
struct Tw { uint32_t *tw = nullptr, *twinv = nullptr, *ninv = nullptr; };
std::mutex g_tw_mu;
Tw g_tw[POLY_MAX_LOG + 1];
int tw_get(int logN, Tw& out) {
  if (logN < 1 || logN > POLY_MAX_LOG) return ZKT_ERR_SHAPE;
  std::lock_guard<std::mutex> lk(g_tw_mu);
  Tw& e = g_tw[logN];
  if (!e.tw) {
    const size_t half = (size_t)1 << (logN - 1);
    void* p = nullptr;
    if (hipMalloc(&p, (2 * half + 1) * FRB) != hipSuccess) { (void)hipGetLastError(); return ZKT_ERR_DEVICE; }
    uint32_t* w = (uint32_t*)p;
    const int rc = fr_ntt_twiddles(logN, w, w + half * FW, w + 2 * half * FW, nullptr);
    if (rc != ZKT_OK) { (void)hipFree(p); return rc; }
    e.tw = w; e.twinv = w + half * FW; e.ninv = w + 2 * half * FW;
  }
  out = e; return ZKT_OK;
}
int log2_ceil(size_t x) { int k = 1; while (((size_t)1 << k) < x) ++k; return k; }       // transform sizes start at 2

template <bool IC, bool OC>
void gather(uint32_t* dst, size_t n, const uint32_t* src, size_t cnt, long long start, int step, const uint32_t* scale, int scale_sq, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_gather<IC, OC>), dim3(grid_blocks(n)), dim3(256), 0, s, dst, n, src, cnt, start, step, scale, scale_sq);
}

// out[0 .. keep) = the low coefficients of a b, keep <= na + nb - 1.  CANON: a, b and out in the caller's layout.  a == b (with na == nb) squares.
template <bool CANON>
int pmul(Pool& pool, const uint32_t* a, size_t na, const uint32_t* b, size_t nb, uint32_t* out, size_t keep) {
  hipStream_t s = pool.s;
  if (keep == 0) return ZKT_OK;
  if ((na < nb ? na : nb) <= POLY_DIRECT_MAX) {
    const bool a_short = na <= nb;
    hipLaunchKernelGGL(k_mul_direct<CANON>, dim3(grid_blocks(keep)), dim3(256), 0, s, a_short ? a : b, a_short ? na : nb, a_short ? b : a, a_short ? nb : na, out, keep);
    HIPCHK(hipGetLastError()); return ZKT_OK;
  }
  const int logN = log2_ceil(na + nb - 1); const size_t N = (size_t)1 << logN;
  Tw tw; ZCHK(tw_get(logN, tw));
  PGET(A, pool, N);
  gather<CANON, false>(A, N, a, na, 0, 1, nullptr, 0, s);
  if (a == b && na == nb) {
    ZCHK(fr_ntt_forward(A, logN, tw.tw, nullptr, s, 1));
    hipLaunchKernelGGL(k_sqr_all, dim3(grid_blocks(N)), dim3(256), 0, s, A, N);
  } else {
    PGET(B, pool, N);
    gather<CANON, false>(B, N, b, nb, 0, 1, nullptr, 0, s);
    ZCHK(fr_ntt_forward(B, logN, tw.tw, nullptr, s, 1));
    ZCHK(fr_ntt_forward(A, logN, tw.tw, B, s, 1));
  }
  ZCHK(fr_ntt_inverse(A, logN, tw.twinv, s, 1));
  gather<false, CANON>(out, keep, A, keep, 0, 1, tw.ninv, 0, s);
  HIPCHK(hipGetLastError()); return ZKT_OK;
}

// g[0 .. L) = 1 / rev(b) mod x^L from g[0] = finv; g has room for 2^ceil(log2 L) elements
int newton_inverse(Pool& pool, const uint32_t* b, size_t nb, uint32_t* g, size_t L) {
  hipStream_t s = pool.s;
  if (L <= 1) return ZKT_OK;
  const size_t Lp = (size_t)1 << log2_ceil(L);
  PGET(T, pool, Lp); PGET(GS, pool, Lp); PGET(E, pool, Lp);
  for (size_t p = 1; p < L; p *= 2) {
    const size_t N = 2 * p; const int logN = log2_ceil(N);
    Tw tw; ZCHK(tw_get(logN, tw));
    gather<false, false>(T, N, b, nb < N ? nb : N, (long long)nb - 1, -1, nullptr, 0, s);        // rev(b) mod x^N
    gather<false, false>(GS, N, g, p, 0, 1, nullptr, 0, s);
    ZCHK(fr_ntt_forward(GS, logN, tw.tw, nullptr, s, 1));
    ZCHK(fr_ntt_forward(T, logN, tw.tw, GS, s, 1));
    ZCHK(fr_ntt_inverse(T, logN, tw.twinv, s, 1));                                         // N (f g mod x^N - 1): coefficients p .. N-1 are N e
    gather<false, false>(E, N, T + p * FW, p, 0, 1, nullptr, 0, s);
    ZCHK(fr_ntt_forward(E, logN, tw.tw, GS, s, 1));
    ZCHK(fr_ntt_inverse(E, logN, tw.twinv, s, 1));                                         // N^2 (e g)
    hipLaunchKernelGGL(k_newton_update, dim3(grid_blocks(p)), dim3(256), 0, s, g + p * FW, (const uint32_t*)E, p, (const uint32_t*)tw.ninv);
  }
  HIPCHK(hipGetLastError()); return ZKT_OK;
}

// q (L = na - nb + 1) and rem (nb - 1) of a / b, all Montgomery device buffers; the leading coefficient of b is non-zero (derr takes nb - 1 if it is not)
int divrem_dev(Pool& pool, const uint32_t* a, size_t na, const uint32_t* b, size_t nb, uint32_t* q, uint32_t* rem, unsigned long long* derr) {
  hipStream_t s = pool.s;
  const size_t L = na - nb + 1;
  if (L <= POLY_DIV_DIRECT_MAX) {
    PGET(finv, pool, 1);
    hipLaunchKernelGGL(k_inv1, dim3(1), dim3(64), 0, s, b + (nb - 1) * FW, finv, derr, (unsigned long long)(nb - 1));
    hipLaunchKernelGGL(k_div_direct, dim3(1), dim3(256), 0, s, a, na, b, nb, q, L, (const uint32_t*)finv);
  } else {
    const size_t Lp = (size_t)1 << log2_ceil(L);
    PGET(g, pool, Lp); PGET(ra, pool, L); PGET(rq, pool, L);
    hipLaunchKernelGGL(k_inv1, dim3(1), dim3(64), 0, s, b + (nb - 1) * FW, g, derr, (unsigned long long)(nb - 1));
    ZCHK(newton_inverse(pool, b, nb, g, L));
    gather<false, false>(ra, L, a, L, (long long)na - 1, -1, nullptr, 0, s);
    if (2 * L - 1 <= ZKT_POLY_MAX_LEN) ZCHK(pmul<false>(pool, ra, L, g, L, rq, L));
    else {      // the full product would need a transform beyond the largest: ra g mod x^L = ra0 g0 + x^h (ra0 g1 + ra1 g0) from three products of halves
      const size_t h = (L + 1) / 2, r = L - h;
      PGET(t1, pool, r); PGET(t2, pool, r);
      gather<false, false>(rq, L, rq, 0, 0, 1, nullptr, 0, s);                         // zeros (2h - 1 may be L - 1)
      ZCHK(pmul<false>(pool, ra, h, g, h, rq, 2 * h - 1 < L ? 2 * h - 1 : L));
      ZCHK(pmul<false>(pool, ra, h, g + h * FW, r, t1, r));
      ZCHK(pmul<false>(pool, ra + h * FW, r, g, h, t2, r));
      hipLaunchKernelGGL(k_add2, dim3(grid_blocks(r)), dim3(256), 0, s, rq + h * FW, (const uint32_t*)t1, (const uint32_t*)t2, r);
    }
    gather<false, false>(q, L, rq, L, (long long)L - 1, -1, nullptr, 0, s);
  }
  const size_t nr = nb - 1;
  if (nr == 0) { HIPCHK(hipGetLastError()); return ZKT_OK; }
  if ((L < nb ? L : nb) <= POLY_DIRECT_MAX) {
    PGET(qb, pool, nr);
    ZCHK(pmul<false>(pool, q, L, b, nb, qb, nr));
    hipLaunchKernelGGL(k_sub<false>, dim3(grid_blocks(nr)), dim3(256), 0, s, rem, a, (const uint32_t*)qb, nr, (const uint32_t*)nullptr);
  } else {
    const int logN = log2_ceil(nr); const size_t N = (size_t)1 << logN;
    Tw tw; ZCHK(tw_get(logN, tw));
    PGET(QF, pool, N); PGET(BF, pool, N); PGET(AF, pool, N);
    hipLaunchKernelGGL(k_fold, dim3(grid_blocks(N)), dim3(256), 0, s, QF, N, (const uint32_t*)q, L);
    hipLaunchKernelGGL(k_fold, dim3(grid_blocks(N)), dim3(256), 0, s, BF, N, b, nb);
    hipLaunchKernelGGL(k_fold, dim3(grid_blocks(N)), dim3(256), 0, s, AF, N, a, na);
    ZCHK(fr_ntt_forward(BF, logN, tw.tw, nullptr, s, 1));
    ZCHK(fr_ntt_forward(QF, logN, tw.tw, BF, s, 1));
    ZCHK(fr_ntt_inverse(QF, logN, tw.twinv, s, 1));
    hipLaunchKernelGGL(k_sub<false>, dim3(grid_blocks(nr)), dim3(256), 0, s, rem, (const uint32_t*)AF, (const uint32_t*)QF, nr, (const uint32_t*)tw.ninv);
  }
  HIPCHK(hipGetLastError()); return ZKT_OK;
}

}  // namespace
// out[0 .. n] = the coefficients of prod_{i=1..n} (x - i), Montgomery (fr_pool.h: zkt_qap.hip divides it by every x - j)
int build_t_dev(Pool& pool, size_t n, uint32_t* out) {
  hipStream_t s = pool.s;
  if (n == 0) {                                            // the empty product
    hipLaunchKernelGGL(k_tree_scatter, dim3(1), dim3(256), 0, s, (const uint32_t*)out, out, (size_t)0, (size_t)0, (size_t)1, (const uint32_t*)out);      // one node of degree 0: its leading 1
    HIPCHK(hipGetLastError()); return ZKT_OK;
  }
  PGET(cur, pool, 2 * n + 4); PGET(nxt, pool, 2 * n + 4);
  hipLaunchKernelGGL(k_tree_leaves, dim3(grid_blocks(n)), dim3(256), 0, s, cur, n);
  uint32_t *X = nullptr, *Y = nullptr;
  for (size_t sp = 1; sp < n; sp *= 2) {
    const size_t nodes = (n + 2 * sp - 1) / (2 * sp), per = 2 * sp + 1;
    if (sp <= POLY_DIRECT_MAX) {
      hipLaunchKernelGGL(k_tree_direct, dim3(grid_blocks(nodes * per)), dim3(256), 0, s, (const uint32_t*)cur, nxt, sp, n, nodes);
    } else {
      const int logN = log2_ceil(2 * sp); const size_t N = 2 * sp;
      Tw tw; ZCHK(tw_get(logN, tw));
      if (!X) { const size_t cap = 2 * n + 2 * POLY_DIRECT_MAX + 4; X = pool.get(cap); Y = pool.get(cap); if (!X || !Y) return ZKT_ERR_DEVICE; }     // nodes * N < n + 2 sp <= 2n at every level
      hipLaunchKernelGGL(k_tree_gather, dim3(grid_blocks(nodes * N)), dim3(256), 0, s, (const uint32_t*)cur, X, Y, sp, n, nodes);
      ZCHK(fr_ntt_forward(Y, logN, tw.tw, nullptr, s, nodes));
      ZCHK(fr_ntt_forward(X, logN, tw.tw, Y, s, nodes));
      ZCHK(fr_ntt_inverse(X, logN, tw.twinv, s, nodes));
      hipLaunchKernelGGL(k_tree_scatter, dim3(grid_blocks(nodes * per)), dim3(256), 0, s, (const uint32_t*)X, nxt, sp, n, nodes, (const uint32_t*)tw.ninv);
    }
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
  gather<false, false>(out, n + 1, cur, n + 1, 0, 1, nullptr, 0, s);
  HIPCHK(hipGetLastError()); return ZKT_OK;
}

namespace {
bool lead_is_zero(const uint64_t* w) {                     // 0, r or 2r: the 256-bit integers that are zero mod r
  static const uint64_t R1[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
  static const uint64_t R2[4] = {0xfffffffe00000002ull, 0xa77b4805fffcb7fdull, 0x6673b0101343b00aull, 0xe7db4ea6533afa90ull};
  return (w[0] | w[1] | w[2] | w[3]) == 0 || memcmp(w, R1, 32) == 0 || memcmp(w, R2, 32) == 0;
}

// h (n - 1, Montgomery) = (U V - W) / t from the three combined polynomials (n coefficients each, Montgomery); *rem_top = 1 + the remainder's degree, 0 when it is zero
int quotient_dev(Pool& pool, const uint32_t* U, const uint32_t* V, const uint32_t* W, size_t n, uint32_t* h, unsigned long long* d_top) {
  hipStream_t s = pool.s;
  PGET(P, pool, 2 * n - 1);
  ZCHK(pmul<false>(pool, U, n, V, n, P, 2 * n - 1));
  hipLaunchKernelGGL(k_sub<false>, dim3(grid_blocks(n)), dim3(256), 0, s, P, (const uint32_t*)P, W, n, (const uint32_t*)nullptr);
  if (n == 1) {                                            // t = x - 1 does not divide a non-zero constant: the remainder is p itself
    hipLaunchKernelGGL(k_top_nonzero, dim3(1), dim3(256), 0, s, (const uint32_t*)P, (size_t)1, d_top);
    HIPCHK(hipGetLastError()); return ZKT_OK;
  }
  PGET(T, pool, n + 1); PGET(rem, pool, n);
  ZCHK(build_t_dev(pool, n, T));
  ZCHK(divrem_dev(pool, P, 2 * n - 1, T, n + 1, h, rem, d_top + 1));
  hipLaunchKernelGGL(k_top_nonzero, dim3(grid_blocks(n)), dim3(256), 0, s, (const uint32_t*)rem, n, d_top);
  HIPCHK(hipGetLastError()); return ZKT_OK;
}

// ui, vi, wi on the device in the caller's layout (rows x n); uploads the wires and leaves U, V, W (Montgomery) and h; returns ZKT_ERR_REMAINDER (+ index) when t does not divide p
int qap_quotient_dev(Pool& pool, const uint32_t* du, const uint32_t* dv, const uint32_t* dwi, size_t rows, size_t n, const uint64_t* wires,
                     uint32_t** U, uint32_t** V, uint32_t** h) {
  hipStream_t s = pool.s;
  PGET(dw, pool, rows);
  PGET(cu, pool, n); PGET(cv, pool, n); PGET(cw, pool, n); PGET(dh, pool, n); PGET(flags, pool, 1);
  HIPCHK(hipMemcpyAsync(dw, wires, rows * FRB, hipMemcpyHostToDevice, s));
  unsigned long long init[2] = {0, NO_ERR}, got[2];         // [0]: 1 + degree of the remainder; [1]: a zero leading coefficient (t is monic: never)
  HIPCHK(hipMemcpyAsync(flags, init, 16, hipMemcpyHostToDevice, s));
  Comb3 c; c.m[0] = du; c.m[1] = dv; c.m[2] = dwi; c.out[0] = cu; c.out[1] = cv; c.out[2] = cw;
  hipLaunchKernelGGL(k_wire_comb, dim3(grid_blocks(n), 3), dim3(256), 0, s, c, (const uint32_t*)dw, rows, n);
  ZCHK(quotient_dev(pool, cu, cv, cw, n, dh, (unsigned long long*)flags));
  HIPCHK(hipMemcpyAsync(got, flags, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (got[0]) { zkt_internal_set_error_index((size_t)got[0] - 1); return ZKT_ERR_REMAINDER; }
  *U = cu; *V = cv; *h = dh;
  return ZKT_OK;
}
// the same from host arrays: their uploads, then qap_quotient_dev
int qap_quotient_host(Pool& pool, const uint64_t* ui, const uint64_t* vi, const uint64_t* wi, size_t rows, size_t n, const uint64_t* wires,
                      uint32_t** U, uint32_t** V, uint32_t** h) {
  hipStream_t s = pool.s;
  PGET(du, pool, rows * n); PGET(dv, pool, rows * n); PGET(dwi, pool, rows * n);
  HIPCHK(hipMemcpyAsync(du, ui, rows * n * FRB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dv, vi, rows * n * FRB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dwi, wi, rows * n * FRB, hipMemcpyHostToDevice, s));
  return qap_quotient_dev(pool, du, dv, dwi, rows, n, wires, U, V, h);
}
}  // namespace
int store_host(uint64_t* dst, const uint32_t* src, size_t cnt, Pool& pool) {         // Montgomery device values -> canonical host words (queued; fr_pool.h)
  if (!cnt) return ZKT_OK;
  PGET(tmp, pool, cnt);
  gather<false, true>(tmp, cnt, src, cnt, 0, 1, nullptr, 0, pool.s);
  HIPCHK(hipMemcpyAsync(dst, tmp, cnt * FRB, hipMemcpyDeviceToHost, pool.s));
  return ZKT_OK;
}
namespace {
bool mul_shape_ok(const void* a, size_t na, const void* b, size_t nb, const void* out) {
  return a && b && out && na && nb && na <= ZKT_POLY_MAX_LEN && nb <= ZKT_POLY_MAX_LEN && na + nb - 1 <= ZKT_POLY_MAX_LEN;
}
}  // namespace
}  // namespace zkt

using namespace zkt;

extern "C" {

void zkt_poly_clear_caches() {
  std::lock_guard<std::mutex> lk(g_tw_mu);
  for (Tw& e : g_tw) { if (e.tw) (void)hipFree(e.tw); e = Tw(); }
}

// Polynomial::multiply_by (polynomial.rs:173-190)
int zkt_fr_poly_mul_dev(const uint64_t* dev_a, size_t na, const uint64_t* dev_b, size_t nb, uint64_t* dev_out, void* stream) {
  if (!mul_shape_ok(dev_a, na, dev_b, nb, dev_out)) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool((hipStream_t)stream);
  return pmul<true>(pool, (const uint32_t*)dev_a, na, (const uint32_t*)dev_b, nb, (uint32_t*)dev_out, na + nb - 1);
}
int zkt_fr_poly_mul(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out) {
  if (!mul_shape_ok(a, na, b, nb, out)) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr); hipStream_t s = nullptr;
  const size_t no = na + nb - 1;
  PGET(da, pool, na); PGET(dout, pool, no);
  uint32_t* db = da;
  HIPCHK(hipMemcpyAsync(da, a, na * FRB, hipMemcpyHostToDevice, s));
  if (!(a == b && na == nb)) { db = pool.get(nb); if (!db) return ZKT_ERR_DEVICE; HIPCHK(hipMemcpyAsync(db, b, nb * FRB, hipMemcpyHostToDevice, s)); }
  ZCHK(pmul<true>(pool, da, na, db, nb, dout, no));
  HIPCHK(hipMemcpyAsync(out, dout, no * FRB, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ZKT_OK;
}

// Polynomial::divide_by (polynomial.rs:204-238)
int zkt_fr_poly_divrem(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* q, uint64_t* rem, size_t* rem_len) {
  if (!a || !b || !q || !rem_len || nb == 0 || (nb > 1 && !rem) || na > ZKT_POLY_MAX_LEN || nb > ZKT_POLY_MAX_LEN) return ZKT_ERR_SHAPE;
  if (na < nb || lead_is_zero(b + (nb - 1) * 4)) { zkt_internal_set_error_index(nb - 1); return ZKT_ERR_SHAPE; }      // :207 underflows, :209 asserts
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr); hipStream_t s = nullptr;
  const size_t L = na - nb + 1, nr = nb - 1;
  PGET(ca, pool, na); PGET(cb, pool, nb); PGET(da, pool, na); PGET(db, pool, nb); PGET(dq, pool, L); PGET(dr, pool, nr); PGET(flags, pool, 1);
  HIPCHK(hipMemcpyAsync(ca, a, na * FRB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(cb, b, nb * FRB, hipMemcpyHostToDevice, s));
  unsigned long long init[2] = {0, NO_ERR}, got[2];
  HIPCHK(hipMemcpyAsync(flags, init, 16, hipMemcpyHostToDevice, s));
  gather<true, false>(da, na, ca, na, 0, 1, nullptr, 0, s);
  gather<true, false>(db, nb, cb, nb, 0, 1, nullptr, 0, s);
  ZCHK(divrem_dev(pool, da, na, db, nb, dq, dr, (unsigned long long*)flags + 1));
  if (nr) hipLaunchKernelGGL(k_top_nonzero, dim3(grid_blocks(nr)), dim3(256), 0, s, (const uint32_t*)dr, nr, (unsigned long long*)flags);
  ZCHK(store_host(q, dq, L, pool)); ZCHK(store_host(rem, dr, nr, pool));
  HIPCHK(hipMemcpyAsync(got, flags, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *rem_len = (size_t)got[0];
  return ZKT_OK;
}

// Polynomial::eval_at (polynomial.rs:240-249) at k points; eval_from_1_to_n (:251-262) is xs = 1..n
int zkt_fr_poly_eval_batch(const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t k, uint64_t* out) {
  if (!coeffs || n == 0 || n > ZKT_POLY_MAX_LEN || (k && (!xs || !out))) return ZKT_ERR_SHAPE;
  if (k == 0) return ZKT_OK;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr); hipStream_t s = nullptr;
  PGET(cc, pool, n); PGET(dc, pool, n); PGET(dx, pool, k); PGET(dout, pool, k);
  HIPCHK(hipMemcpyAsync(cc, coeffs, n * FRB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dx, xs, k * FRB, hipMemcpyHostToDevice, s));
  gather<true, false>(dc, n, cc, n, 0, 1, nullptr, 0, s);
  if (n >= EVAL_SPLIT_MIN_N && k < EVAL_SPLIT_MAX_K) {
    const size_t chunks = (n + EVAL_CHUNK - 1) / EVAL_CHUNK;
    PGET(part, pool, k * chunks);
    hipLaunchKernelGGL(k_eval_split, dim3((unsigned)chunks, (unsigned)k), dim3(EVAL_TPB), 0, s, (const uint32_t*)dc, n, (const uint32_t*)dx, chunks, part);
    hipLaunchKernelGGL(k_eval_combine, dim3(grid_blocks(k)), dim3(256), 0, s, (const uint32_t*)part, chunks, (const uint32_t*)dx, k, dout);
  } else {
    hipLaunchKernelGGL(k_eval_horner, dim3(grid_blocks(k)), dim3(256), 0, s, (const uint32_t*)dc, n, (const uint32_t*)dx, k, dout);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout, k * FRB, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ZKT_OK;
}

// QAP::build_t (qap.rs:115-135)
int zkt_qap_build_t(size_t n, uint64_t* out) {
  if (!out || n + 1 > ZKT_POLY_MAX_LEN) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr);
  PGET(T, pool, n + 1);
  ZCHK(build_t_dev(pool, n, T));
  ZCHK(store_host(out, T, n + 1, pool));
  HIPCHK(hipStreamSynchronize(pool.s));
  return ZKT_OK;
}

// QAP::build_p (qap.rs:99-112) and divide_by t (prover.rs:64-71; pinocchio/prover.rs:50-96 with vi, wi, yi)
int zkt_qap_quotient(const uint64_t* ui, const uint64_t* vi, const uint64_t* wi, size_t rows, size_t n, const uint64_t* wires, uint64_t* h) {
  if (!ui || !vi || !wi || !wires || rows == 0 || n == 0 || (n > 1 && !h) || 2 * n - 1 > ZKT_POLY_MAX_LEN || rows > ZKT_POLY_MAX_LEN) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr);
  uint32_t *U, *V, *dh;
  ZCHK(qap_quotient_host(pool, ui, vi, wi, rows, n, wires, &U, &V, &dh));
  ZCHK(store_host(h, dh, n - 1, pool));
  HIPCHK(hipStreamSynchronize(pool.s));
  return ZKT_OK;
}

// QAP::is_valid / Prover::new on a resident QAP (qap.rs:99-112, prover.rs:64-71): zkt_qap_quotient with the three arrays read from the handle
int zkt_qap_quotient_resident(const zkt_qap* q, const uint64_t* wires, uint64_t* h) {
  if (!q || !wires || (q->n > 1 && !h) || 2 * q->n - 1 > ZKT_POLY_MAX_LEN || q->cols > ZKT_POLY_MAX_LEN) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  Pool pool(nullptr);
  uint32_t *U, *V, *dh;
  ZCHK(qap_quotient_dev(pool, q->m[0], q->m[1], q->m[2], q->cols, q->n, wires, &U, &V, &dh));
  ZCHK(store_host(h, dh, q->n - 1, pool));
  HIPCHK(hipStreamSynchronize(pool.s));
  return ZKT_OK;
}

}  // extern "C"

namespace {
bool prove_qap_shape_ok(const zkt_groth16_crs* c, const void* wires, const void* r, const void* s_, const void* A, const void* B, const void* C) {
  return c && wires && r && s_ && A && B && C && c->n != 0 && c->l <= c->m && 2 * c->n - 1 <= ZKT_POLY_MAX_LEN && c->m + 1 <= ZKT_POLY_MAX_LEN;
}
// Prover::new + Prover::prove (prover.rs:50-147): the quotient on the device (from host arrays, or from device arrays when du is given), then the sums and single
// multiplications exactly as zkt_groth16_prove forms them
int prove_qap(const zkt_groth16_crs* c, const uint64_t* ui, const uint64_t* vi, const uint64_t* wi, const uint32_t* du, const uint32_t* dv, const uint32_t* dwi,
              const uint64_t* wires, const uint64_t* r, const uint64_t* s_, zkt_g1_affine* A, zkt_g2_affine* B, zkt_g1_affine* C) {
  const size_t n = c->n, l = c->l, m = c->m, rows = m + 1, nw = m - l;
  std::vector<uint64_t> U(n * 4), V(n * 4), H((n > 1 ? n - 1 : 1) * 4);
  {
    Pool pool(nullptr);
    uint32_t *dU, *dV, *dh;
    if (du) ZCHK(qap_quotient_dev(pool, du, dv, dwi, rows, n, wires, &dU, &dV, &dh));
    else ZCHK(qap_quotient_host(pool, ui, vi, wi, rows, n, wires, &dU, &dV, &dh));
    ZCHK(store_host(U.data(), dU, n, pool)); ZCHK(store_host(V.data(), dV, n, pool)); ZCHK(store_host(H.data(), dh, n - 1, pool));
    HIPCHK(hipStreamSynchronize(pool.s));
  }
  int rc;
  zkt_g1_affine sumA, sumB1, sumW, ht, oA, oC; zkt_g2_affine sumB, oB;
  if ((rc = zkt_g1_msm(c->g1_xi, U.data(), n, &sumA)) || (rc = zkt_g2_msm(c->g2_xi, V.data(), n, &sumB)) || (rc = zkt_g1_msm(c->g1_xi, V.data(), n, &sumB1))) return rc;
  if ((rc = zkt_g1_msm(c->g1_uvw_wit, wires + (l + 1) * 4, nw, &sumW)) || (rc = zkt_g1_msm(c->g1_xt_by_delta, H.data(), n - 1, &ht))) return rc;
  zkt_g1_affine dr, ds, As, Br, drs, t1, t2;
  if ((rc = zkt_g1_mul_batch(c->g1_delta, r, 4, &dr, 1)) || (rc = zkt_g1_mul_batch(c->g1_delta, s_, 4, &ds, 1))) return rc;
  zkt_g2_affine d2s; if ((rc = zkt_g2_mul_batch(c->g2_delta, s_, 4, &d2s, 1))) return rc;
  if ((rc = zkt_g1_add_batch(c->g1_alpha, &sumA, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &dr, &oA, 1))) return rc;                   // A
  zkt_g2_affine t3; if ((rc = zkt_g2_add_batch(c->g2_beta, &sumB, &t3, 1)) || (rc = zkt_g2_add_batch(&t3, &d2s, &oB, 1))) return rc;   // B
  zkt_g1_affine B1; if ((rc = zkt_g1_add_batch(c->g1_beta, &sumB1, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &ds, &B1, 1))) return rc;   // B_g1
  if ((rc = zkt_g1_mul_batch(&oA, s_, 4, &As, 1)) || (rc = zkt_g1_mul_batch(&B1, r, 4, &Br, 1)) || (rc = zkt_g1_mul_batch(&dr, s_, 4, &drs, 1))) return rc;
  zkt_g1_affine ndrs; if ((rc = zkt_g1_neg_batch(&drs, &ndrs, 1))) return rc;
  if ((rc = zkt_g1_add_batch(&sumW, &ht, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &As, &t2, 1)) || (rc = zkt_g1_add_batch(&t2, &Br, &t1, 1)) ||
      (rc = zkt_g1_add_batch(&t1, &ndrs, &oC, 1))) return rc;                                                                          // C
  *A = oA; *B = oB; *C = oC;
  return ZKT_OK;
}
}  // namespace

extern "C" {

int zkt_groth16_prove_qap(const zkt_groth16_crs* c, const uint64_t* ui, const uint64_t* vi, const uint64_t* wi, const uint64_t* wires,
                          const uint64_t* r, const uint64_t* s_, zkt_g1_affine* A, zkt_g2_affine* B, zkt_g1_affine* C) {
  if (!ui || !vi || !wi || !prove_qap_shape_ok(c, wires, r, s_, A, B, C)) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  return prove_qap(c, ui, vi, wi, nullptr, nullptr, nullptr, wires, r, s_, A, B, C);
}
// the same with ui, vi, wi read from a resident QAP
int zkt_groth16_prove_resident(const zkt_groth16_crs* c, const zkt_qap* q, const uint64_t* wires, const uint64_t* r, const uint64_t* s_,
                               zkt_g1_affine* A, zkt_g2_affine* B, zkt_g1_affine* C) {
  if (!q || !prove_qap_shape_ok(c, wires, r, s_, A, B, C) || q->n != c->n || q->cols != c->m + 1) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  return prove_qap(c, nullptr, nullptr, nullptr, q->m[0], q->m[1], q->m[2], wires, r, s_, A, B, C);
}

}  // extern "C"
