// Vectors of Fr elements on the device: the helpers every Fr kernel file shares (and the one block sum of the scalar-field kernels), and the host interface of zkt_fr_vec.hip (transform, prefix product, row-wise Horner).
// An element is FW u32 words, canonical in the caller's layout or Montgomery in the library's own buffers.
#pragma once
#include <hip/hip_runtime.h>
#include "abi.h"

namespace zkt {
typedef Fp<FrC> Fr;
static constexpr int FW = 8;          // u32 words of an Fr element (canonical and Montgomery alike)

// Montgomery in memory, two forms that compile differently: word by word, and as two 128-bit moves (as k_ntt_group moves its tiles).  A kernel keeps the form it was measured with.
__device__ inline Fr ldm(const uint32_t* p) { return ld_raw<FrC>(p); }
__device__ inline void stm(uint32_t* p, const Fr& a) { st_raw<FrC>(p, a); }
__device__ inline Fr ldm4(const uint32_t* p) {
  const uint4* s = reinterpret_cast<const uint4*>(p); const uint4 a = s[0], b = s[1]; Fr r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w; return r;
}
__device__ inline void stm4(uint32_t* p, const Fr& a) {
  uint4* d = reinterpret_cast<uint4*>(p);
  d[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]); d[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
// the integer x as the Montgomery value x R (what fp_from_words does to canonical words)
__device__ inline Fr to_mont(const Fr& x) { uint32_t w[FW];
#pragma unroll
  for (int i = 0; i < FW; ++i) w[i] = x.v[i];
  return fp_from_words<FrC>(w); }
__device__ inline Fr from_mont(const Fr& x) { uint32_t w[FW]; fp_to_words(x, w); Fr r;
#pragma unroll
  for (int i = 0; i < FW; ++i) r.v[i] = w[i];
  return r; }
// CANON: the caller's layout (any 256-bit integer on load, the canonical residue on store); otherwise Montgomery
template <bool CANON> __device__ inline Fr ldx(const uint32_t* p) { Fr x = ldm4(p); return CANON ? to_mont(x) : x; }
template <bool CANON> __device__ inline void stx(uint32_t* p, const Fr& a) { stm4(p, CANON ? from_mont(a) : a); }
__device__ inline Fr fr_small(uint32_t k) { uint32_t w[8] = {k, 0, 0, 0, 0, 0, 0, 0}; return fp_from_words<FrC>(w); }
// t(x) = prod_{k=1..n} (x - k), one lane  (QAP::build_t(f, n).eval_at(x), qap.rs:115-135)
__device__ inline Fr fr_t_at(const Fr& x, size_t n) {
  Fr one = fp_one<FrC>(), t = one, k = fp_zero<FrC>();
  for (size_t i = 1; i <= n; ++i) { k = fp_add(k, one); t = fp_mul(t, fp_sub(x, k)); }
  return t;
}
// Sum of one element per lane over a block of 256 lanes, any of the prime fields: an LDS tree through lds (256 * C::N words).  The sum is valid in thread 0;
// ends on a barrier, so the caller may reuse lds at once.
template <class C> __device__ inline Fp<C> block_sum_256(uint32_t* lds, Fp<C> acc) {
  const int t = threadIdx.x;
  st_raw<C>(lds + t * C::N, acc); __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (t < d) { acc = fp_add(acc, ld_raw<C>(lds + (t + d) * C::N)); st_raw<C>(lds + t * C::N, acc); }
    __syncthreads();
  }
  return acc;
}

// ---- zkt_fr_vec.hip.  Device pointers to Montgomery elements unless said otherwise; each returns a ZKT_* status ----
// forward: natural order in, bit-reversed spectrum out, times `mulvec` (same order) when given; inverse: the reverse, WITHOUT the 1/N.
// `batch` consecutive transforms per array, `ny` arrays `ystride` elements apart.
int fr_ntt_forward(uint32_t* a, int logN, const uint32_t* tw, const uint32_t* mulvec, hipStream_t s, size_t batch = 1, unsigned ny = 1, size_t ystride = 0);
int fr_ntt_inverse(uint32_t* a, int logN, const uint32_t* twinv, hipStream_t s, size_t batch = 1, unsigned ny = 1, size_t ystride = 0);
// tw[k] = w^k and twinv[k] = w^-k for k < N/2, w of order N = 2^logN, and *ninv = 1/N; allocates and waits for s
int fr_ntt_twiddles(int logN, uint32_t* tw, uint32_t* twinv, uint32_t* ninv, hipStream_t s);
// inclusive prefix product, in place allowed (in == out); allocates and waits for s
int fr_scan_mul(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);
// out[i] = P_i(x) for `rows` dense polynomials of n canonical coefficients, x canonical, out Montgomery (Polynomial::eval_at, polynomial.rs:240-249); queued on s
void fr_eval_rows(const uint32_t* P, size_t rows, size_t n, const uint32_t* x, uint32_t* out_mont, hipStream_t s);
}  // namespace zkt
