// Vectors of Fr elements in HBM (fr_vec.h): the NTT of size 2^logN with its twiddle tables, the inclusive prefix product, and row-wise Horner evaluation.
// Callers: the quotient stage and the CRS tables of zkt_groth16_r1cs.hip, the dense polynomials of zkt_poly.hip, the two dense setups (zkt_groth16.hip, zkt_pinocchio.hip).
#include "fr_vec.h"
#include "host_abi.h"

namespace zkt {
typedef FrC C;

// out[0] = 1, out[k>0] = w   (prefix product = w^k)
__global__ void __launch_bounds__(256) k_fill_pow(const uint32_t* __restrict__ w, uint32_t* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  stm(out + i * FW, i ? ldm(w) : fp_one<C>());
}

// ---- inclusive prefix product (factorials, prod (x - j), twiddle tables) ------------------------------------------
static constexpr int SC_TPB = 256, SC_ITEMS = 8, SC_TILE = SC_TPB * SC_ITEMS;
__global__ void __launch_bounds__(SC_TPB) k_scanmul_tile(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n, uint32_t* __restrict__ tile_total) {
  __shared__ uint32_t lds[SC_TPB * FW];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * SC_TILE + (size_t)t * SC_ITEMS;
  Fr loc[SC_ITEMS]; Fr run = fp_one<C>();
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) { if (base + k < n) run = fp_mul(run, ldm(in + (base + k) * FW)); loc[k] = run; }
  stm(lds + t * FW, run); __syncthreads();
  for (int d = 1; d < SC_TPB; d <<= 1) {                 // Hillis-Steele over the 256 thread totals
    Fr o = t >= d ? ldm(lds + (t - d) * FW) : fp_one<C>(); __syncthreads();
    if (t >= d) { run = fp_mul(o, run); stm(lds + t * FW, run); } __syncthreads();
  }
  Fr excl = t ? ldm(lds + (t - 1) * FW) : fp_one<C>();
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) if (base + k < n) stm(out + (base + k) * FW, fp_mul(excl, loc[k]));
  if (t == SC_TPB - 1) stm(tile_total + (size_t)blockIdx.x * FW, run);
}
__global__ void __launch_bounds__(256) k_scanmul_apply(uint32_t* __restrict__ data, size_t n, const uint32_t* __restrict__ tile_prefix) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  size_t tile = i / SC_TILE; if (tile == 0) return;
  stm(data + i * FW, fp_mul(ldm(tile_prefix + (tile - 1) * FW), ldm(data + i * FW)));
}

// ---- Fr NTT of size N = 2^logN ------------------------------------------------------------------------------------
// forward = decimation in frequency (natural order in, bit-reversed out); inverse = decimation in time on the
// bit-reversed spectrum (natural order out), so no reordering pass exists; the 1/N is left to the caller (the R1CS prover keeps it in its precomputed kernel spectrum).
// HBM-bound (one butterfly = one Fr multiply per 64 B moved), so stages are fused through LDS: a launch runs `cnt`
// consecutive radix-2 stages (butterfly distances 2^lo .. 2^(lo+cnt-1)) on a tile of 2^cnt strided rows x 2^cbits
// adjacent columns (<= 1024 elements, 32 KB), every element read and written once per launch, rows of >= 128 B contiguous.
// logN = 21 is three launches per transform (10 + 8 + 3 stages) instead of 21.
// A launch covers any number of transforms of the same size: consecutive ones simply continue blockIdx.x (the twiddle of a butterfly depends on its position
// inside its group only), blockIdx.y steps over arrays `ystride` elements apart.  `mulvec` is indexed like the consecutive transforms of one array.
// (one-wave workgroups for the transform were measured at the end of round 3, in case its four-wave workgroups were what starved beside an accumulate grid: 9.1 ms against 7.6
// for a shard of a proof, 40 against 50 proofs/s on one GPU — not that)
static constexpr int NTT_TILE_LOG = 10, NTT_TPB = 256;
template <bool DIF>
__global__ void __launch_bounds__(NTT_TPB) k_ntt_group(uint32_t* __restrict__ a, int logN, int lo, int cnt, int cbits, const uint32_t* __restrict__ tw,
                                                       const uint32_t* __restrict__ mulvec, size_t ystride) {
  __shared__ uint32_t lds[(1 << NTT_TILE_LOG) * FW];
  a += (size_t)blockIdx.y * ystride * FW;                         // grid.y: independent arrays (the three polynomials), sharing `mulvec`
  const int tile = 1 << (cnt + cbits), cmask = (1 << cbits) - 1;
  const size_t tiles_per_hi = (size_t)1 << (lo - cbits);
  const size_t hi = blockIdx.x / tiles_per_hi, c0 = (blockIdx.x % tiles_per_hi) << cbits;
  const size_t gbase = (hi << (lo + cnt)) | c0;
  for (int e = threadIdx.x; e < tile; e += NTT_TPB) {
    const size_t g = gbase | ((size_t)(e >> cbits) << lo) | (size_t)(e & cmask);
    const uint4* src = reinterpret_cast<const uint4*>(a + g * FW);
    uint4* dst = reinterpret_cast<uint4*>(lds + e * FW);
    dst[0] = src[0]; dst[1] = src[1];
  }
  __syncthreads();
  for (int st = 0; st < cnt; ++st) {
    const int t = DIF ? cnt - 1 - st : st;                       // local butterfly distance 2^t rows
    for (int b = threadIdx.x; b < tile / 2; b += NTT_TPB) {
      const int cc = b & cmask, kb = b >> cbits;
      const int k0 = ((kb >> t) << (t + 1)) | (kb & ((1 << t) - 1));
      const int e0 = (k0 << cbits) | cc, e1 = e0 + (1 << (t + cbits));
      const size_t j = ((size_t)(k0 & ((1 << t) - 1)) << lo) | c0 | (size_t)cc;      // position inside the butterfly group
      const Fr w = ldm(tw + (j << (logN - 1 - lo - t)) * FW);
      Fr u = ldm(lds + e0 * FW), v = ldm(lds + e1 * FW);
      if (DIF) { stm(lds + e0 * FW, fp_add(u, v)); stm(lds + e1 * FW, fp_mul(fp_sub(u, v), w)); }
      else { v = fp_mul(v, w); stm(lds + e0 * FW, fp_add(u, v)); stm(lds + e1 * FW, fp_sub(u, v)); }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < tile; e += NTT_TPB) {
    const size_t g = gbase | ((size_t)(e >> cbits) << lo) | (size_t)(e & cmask);
    if (mulvec) stm(a + g * FW, fp_mul(ldm(lds + e * FW), ldm(mulvec + g * FW)));      // fused pointwise product with a spectrum
    else {
      const uint4* src = reinterpret_cast<const uint4*>(lds + e * FW);
      uint4* dst = reinterpret_cast<uint4*>(a + g * FW);
      dst[0] = src[0]; dst[1] = src[1];
    }
  }
}
// one lane: c = {w, 1/w} for w of order 2^logN, and *ninv = 2^-logN
__global__ void k_ntt_consts(int logN, uint32_t* __restrict__ c, uint32_t* __restrict__ ninv) {
  if (threadIdx.x || blockIdx.x) return;
  uint32_t rw[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) rw[i] = fr_root_word(i);
  Fr w = fp_from_words<C>(rw);
  for (int k = FR_TWO_ADICITY; k > logN; --k) w = fp_sqr(w);                      // order 2^logN
  stm(c, w); stm(c + FW, fp_inv(w));
  Fr two = fr_small(2), nn = fp_one<C>();
  for (int k = 0; k < logN; ++k) nn = fp_mul(nn, two);
  stm(ninv, fp_inv(nn));
}
__global__ void __launch_bounds__(64) k_eval_rows(const uint32_t* __restrict__ P, size_t rows, size_t n, const uint32_t* __restrict__ x, uint32_t* __restrict__ out_mont) {
  size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= rows) return;
  Fp<C> xm = ld_fp<C>(x), acc = fp_zero<C>();
  for (size_t k = n; k-- > 0;) acc = fp_add(fp_mul(acc, xm), ld_fp<C>(P + (i * n + k) * C::N));     // Horner, Montgomery domain
  st_raw<C>(out_mont + i * C::N, acc);
}

// two levels of tiles cover 2048^2 elements
int fr_scan_mul(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
  if (n == 0) return ZKT_OK;
  const size_t tiles = (n + SC_TILE - 1) / SC_TILE;
  if (tiles > (size_t)SC_TILE) return ZKT_ERR_SHAPE;
  Dev tot, tot2; ZCHK(tot.alloc(tiles * FRB)); ZCHK(tot2.alloc(FRB));
  hipLaunchKernelGGL(k_scanmul_tile, dim3((unsigned)tiles), dim3(SC_TPB), 0, s, in, out, n, tot.w());
  if (tiles > 1) {
    hipLaunchKernelGGL(k_scanmul_tile, dim3(1), dim3(SC_TPB), 0, s, (const uint32_t*)tot.w(), tot.w(), tiles, tot2.w());
    hipLaunchKernelGGL(k_scanmul_apply, dim3(grid_blocks(n)), dim3(256), 0, s, out, n, (const uint32_t*)tot.w());
  }
  HIPCHK(hipStreamSynchronize(s));     // the tile totals die with this frame
  return ZKT_OK;
}
// stage groups: the contiguous one first (distances 1..2^(c0-1)), then strided groups of <= 8 stages with >= 4 adjacent columns
struct NttGroup { int lo, cnt, cbits; };
static int ntt_groups(int logN, NttGroup* g) {
  int k = 0, c0 = logN < NTT_TILE_LOG ? logN : NTT_TILE_LOG;
  g[k++] = {0, c0, 0};
  for (int lo = c0, rem = logN - c0; rem > 0;) {
    int cnt = rem < 8 ? rem : 8, cb = NTT_TILE_LOG - cnt; if (cb > lo) cb = lo;
    g[k++] = {lo, cnt, cb}; lo += cnt; rem -= cnt;
  }
  return k;
}
int fr_ntt_forward(uint32_t* a, int logN, const uint32_t* tw, const uint32_t* mulvec, hipStream_t s, size_t batch, unsigned ny, size_t ystride) {
  NttGroup g[8]; const int k = ntt_groups(logN, g);
  for (int i = k - 1; i >= 0; --i)
    hipLaunchKernelGGL(k_ntt_group<true>, dim3((unsigned)((batch << logN) >> (g[i].cnt + g[i].cbits)), ny), dim3(NTT_TPB), 0, s, a, logN, g[i].lo, g[i].cnt, g[i].cbits, tw,
                       i == 0 ? mulvec : (const uint32_t*)nullptr, ystride);
  HIPCHK(hipGetLastError()); return ZKT_OK;
}
int fr_ntt_inverse(uint32_t* a, int logN, const uint32_t* twinv, hipStream_t s, size_t batch, unsigned ny, size_t ystride) {
  NttGroup g[8]; const int k = ntt_groups(logN, g);
  for (int i = 0; i < k; ++i)
    hipLaunchKernelGGL(k_ntt_group<false>, dim3((unsigned)((batch << logN) >> (g[i].cnt + g[i].cbits)), ny), dim3(NTT_TPB), 0, s, a, logN, g[i].lo, g[i].cnt, g[i].cbits, twinv,
                       (const uint32_t*)nullptr, ystride);
  HIPCHK(hipGetLastError()); return ZKT_OK;
}
int fr_ntt_twiddles(int logN, uint32_t* tw, uint32_t* twinv, uint32_t* ninv, hipStream_t s) {
  if (logN < 1 || logN > FR_TWO_ADICITY) return ZKT_ERR_SHAPE;
  const size_t half = (size_t)1 << (logN - 1);
  Dev c; ZCHK(c.alloc(2 * FRB));
  hipLaunchKernelGGL(k_ntt_consts, dim3(1), dim3(64), 0, s, logN, c.w(), ninv);
  hipLaunchKernelGGL(k_fill_pow, dim3(grid_blocks(half)), dim3(256), 0, s, (const uint32_t*)c.w(), tw, half);
  ZCHK(fr_scan_mul(tw, tw, half, s));
  hipLaunchKernelGGL(k_fill_pow, dim3(grid_blocks(half)), dim3(256), 0, s, (const uint32_t*)(c.w() + FW), twinv, half);
  return fr_scan_mul(twinv, twinv, half, s);       // waits for s: `c` dies with this frame
}
void fr_eval_rows(const uint32_t* P, size_t rows, size_t n, const uint32_t* x, uint32_t* out_mont, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_rows, dim3(grid_blocks(rows, 64)), dim3(64), 0, s, P, rows, n, x, out_mont);
}
}  // namespace zkt
