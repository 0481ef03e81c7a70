// G1 multi-scalar multiplication  sum_i s_i * P_i  for gfx950 (row a9 of SURVEY §8).
//   Polynomial::eval_with_g1_hidings   src/building_block/field/polynomial.rs:271-281
// The reference runs n double-and-add scalar multiplications and n affine additions
// strictly sequentially.  The group element is the same whatever the summation order,
// and the result leaves as a canonical affine point, so this is bit-compatible.
//
// MI355X-first design:
//  * bases are device-resident (a CRS is uploaded once and reused by every proof) and,
//    because HBM is 288 GB, every base is stored together with its window multiples
//    2^(c*w) * P_i  (nwin * n affine points, 112 B each for G1).  All windows then share ONE set
//    of 2^(c-1) buckets: there is no per-window bucket reduction and no final Horner
//    chain of 256 serial doublings — on this machine a serial Fq multiply costs ~1.1 us
//    per lane, so serial chains, not FLOPs, are what must be designed away.
//  * signed c-bit digits (scalars used as-is, 256 bits: macros.rs:10-21), counting sort of
//    (bucket, point) pairs, one bucket per lane accumulating in XYZZ coordinates with
//    complete mixed additions (P+P, P+(-P), infinity: macros.rs:43-63), gather of 112-byte
//    affine points, then a two-level bucket reduction built from short trees.
//  * one-shot calls with host pointers use the DIRECT form instead (msm_plan_direct): no table, every window owns its
//    buckets, all windows are reduced side by side (grid.y) and joined by one wave — the serial doubling chain is paid once
//    per call instead of a table build that costs 40x a resident MSM.
#include "abi.h"
#include "msm_ws.h"

namespace zkt {

// The pipeline is generic over the group: G1 over Fq (FqOps), G2 over Fq2 (Fq2Ops, row f-1: eval_with_g2_hidings,
// polynomial.rs:283-293) and secp256k1 (SpOps: (AffinePoints * PrimeFieldElems).sum(), secp256k1/affine_points.rs:25-31,123-144).
// This file is compiled once per group (Makefile): the stages that depend on the group are here, the sort stage is msm_sort.h and the bucket reduction
// msm_reduce_coop.h; the plans and the workspace are zkt_msm_plan.cpp, the by-group entry points zkt_msm_dispatch.cpp.
// Coordinates are stored raw (Montgomery, in the limb layout of the object's field) with CW words each: affine point = 2*CW, XYZZ = 4*CW, Jacobian partial = 3*CW.
// Words of a coordinate IN MEMORY (CW) are not the limbs of its field: the G1 object may run Fq on 13 x 30-bit limbs (Fq30C, -DZKT_FQ30) in the 14-word slots of
// the 14 x 28 layout, so that every size the host code knows (table entries, bucket sums, the 42-word Jacobian partial of include/zkt.h) is the same for both.
// A store writes the words past the limbs as zero; a load does not read them.
template <class C> struct CoordMemWords { static constexpr int value = C::N; };
template <> struct CoordMemWords<Fq30C> { static constexpr int value = FqC::N; };
#if defined(ZKT_FQ30)
typedef PrimeOps<Fq30C> G1Ops;
#else
typedef FqOps G1Ops;
#endif
template <class F> struct Coord;
template <class C> struct Coord<PrimeOps<C>> {
  static constexpr int CW = CoordMemWords<C>::value;
  __device__ static Fp<C> ld(const uint32_t* p) { return ld_raw<C>(p); }
  __device__ static void st(uint32_t* p, const Fp<C>& a) {
    st_raw<C>(p, a);
#pragma unroll
    for (int i = C::N; i < CW; ++i) p[i] = 0u;
  }
};
template <> struct Coord<Fq2Ops> {
  static constexpr int CW = 2 * FqC::N;
  __device__ static Fq2 ld(const uint32_t* p) { Fq2 r; r.c0 = ld_raw<FqC>(p); r.c1 = ld_raw<FqC>(p + FqC::N); return r; }
  __device__ static void st(uint32_t* p, const Fq2& a) { st_raw<FqC>(p, a.c0); st_raw<FqC>(p + FqC::N, a.c1); }
};
template <class F> __device__ inline Xyzz<F> ld_xy(const uint32_t* p) {
  constexpr int CW = Coord<F>::CW; Xyzz<F> r;
  r.X = Coord<F>::ld(p); r.Y = Coord<F>::ld(p + CW); r.ZZ = Coord<F>::ld(p + 2 * CW); r.ZZZ = Coord<F>::ld(p + 3 * CW); return r;
}
template <class F> __device__ inline void st_xy(uint32_t* p, const Xyzz<F>& a) {
  constexpr int CW = Coord<F>::CW;
  Coord<F>::st(p, a.X); Coord<F>::st(p + CW, a.Y); Coord<F>::st(p + 2 * CW, a.ZZ); Coord<F>::st(p + 3 * CW, a.ZZZ);
}

// ---- layout conversion and window-multiple precomputation ----
template <class F>
__global__ void __launch_bounds__(64) k_to_kernel_layout(const uint32_t* __restrict__ abi, uint32_t* __restrict__ mont,
                                                         uint8_t* __restrict__ inf, size_t n) {
  size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int CW = Coord<F>::CW;
  Aff<F> p = PtIO<F>::ld(abi + i * PtIO<F>::WORDS);
  Coord<F>::st(mont + i * 2 * CW, p.x); Coord<F>::st(mont + i * 2 * CW + CW, p.y);
  inf[i] = p.inf ? 1 : 0;
}
// This file is compiled three times (Makefile), and each build selects its group here: -DZKT_MSM_PART_G1 -DZKT_INLINE_MUL instantiates the G1 kernels with the
// field multiply inlined (the headline path); -DZKT_MSM_PART_SECP -DZKT_INLINE_MUL does the same for secp256k1 (8-limb field: small code; a called multiply is
// latency bound at the low occupancy of 2^17-term MSMs); -DZKT_MSM_PART_OTHER instantiates G2 with a called multiply (an inlined Fq2 XYZZ add would be ~200 KB of
// code and minutes of compile time).  GF is the object's field, GRP its group id, MSM_LAUNCHERS the table of its launchers (at the end of the file).
#if defined(ZKT_MSM_PART_G1)
typedef G1Ops GF; static constexpr int GRP = G_G1;
#define MSM_LAUNCHERS msm_launchers_g1
#elif defined(ZKT_MSM_PART_SECP)
typedef SpOps GF; static constexpr int GRP = G_SECP;
#define MSM_LAUNCHERS msm_launchers_secp
#else
typedef Fq2Ops GF; static constexpr int GRP = G_G2;
#define MSM_LAUNCHERS msm_launchers_g2
#endif
static_assert(Coord<GF>::CW == coord_words(GRP), "the host code sizes tables and workspaces by coord_words (msm_ws.h)");

static hipError_t launch_to_kernel_layout(int grp, const uint32_t* abi, uint32_t* mont, uint8_t* inf, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (grp != GRP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_to_kernel_layout<GF>, dim3(grid_blocks(n, 64)), dim3(64), 0, s, abi, mont, inf, n);
  return hipGetLastError();
}

// table[w*n + i] = 2^(c*w) * P_i (affine, Montgomery); infinity flags likewise.
// One lane walks one point through all windows in Jacobian coordinates (255 doublings) and normalises the nwin-1 results with ONE
// inversion (Montgomery's trick along the lane's own chain): X_w, Y_w wait in their table slots, Z_w and prod_{v<w} Z_v in `tmp`
// (two coordinates per entry, freed after the build).  An inversion per window made the build 3x longer than the doublings alone.
template <class F>
__global__ void __launch_bounds__(64) k_precompute(uint32_t* __restrict__ table, uint8_t* __restrict__ inf, size_t n, int c, int nwin, uint32_t* __restrict__ tmp) {
  size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || nwin < 2) return;
  constexpr int CW = Coord<F>::CW, PW = 2 * CW;
  typedef typename F::E E;
  Aff<F> a; a.x = Coord<F>::ld(table + i * PW); a.y = Coord<F>::ld(table + i * PW + CW); a.inf = inf[i] != 0;
  Jac<F> j = jac_from_aff(a);
  E acc = F::one();
  for (int w = 1; w < nwin; ++w) {
    for (int d = 0; d < c; ++d) j = jac_dbl(j);
    const size_t o = (size_t)w * n + i, t = (size_t)(w - 1) * n + i;
    const bool isinf = jac_is_inf(j);
    const E z = isinf ? F::one() : j.Z;
    Coord<F>::st(table + o * PW, j.X); Coord<F>::st(table + o * PW + CW, j.Y);
    Coord<F>::st(tmp + t * PW, z); Coord<F>::st(tmp + t * PW + CW, acc);
    inf[o] = isinf ? 1 : 0;
    acc = F::mul(acc, z);
  }
  E inv = F::inv(acc);                                      // 1 / (Z_1 ... Z_{nwin-1}), no factor is zero
  for (int w = nwin - 1; w >= 1; --w) {
    const size_t o = (size_t)w * n + i, t = (size_t)(w - 1) * n + i;
    const E z = Coord<F>::ld(tmp + t * PW), pre = Coord<F>::ld(tmp + t * PW + CW);
    const E zi = F::mul(inv, pre);                          // 1 / Z_w
    inv = F::mul(inv, z);
    const E zi2 = F::sqr(zi);
    E x = F::mul(Coord<F>::ld(table + o * PW), zi2), y = F::mul(Coord<F>::ld(table + o * PW + CW), F::mul(zi2, zi));
    if (inf[o]) { x = F::zero(); y = F::zero(); }
    Coord<F>::st(table + o * PW, x); Coord<F>::st(table + o * PW + CW, y);
  }
}

// ---- stage 1: signed digits, counting sort by bucket, task list: msm_sort.h (nothing in it depends on the group) ----
}  // namespace zkt
#include "msm_sort.h"
namespace zkt {

// ---- bucket accumulation: one task (bucket chunk) per lane — the dominant kernel ----
#ifndef ZKT_ACC_ATTR
#define ZKT_ACC_ATTR
#endif
template <class F>
__global__ void __launch_bounds__(64) ZKT_ACC_ATTR k_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ entries,
                                                   const uint32_t* __restrict__ offsets, const uint2* __restrict__ order,
                                                   const uint32_t* __restrict__ task_off, size_t nbuckets,
                                                   uint32_t* __restrict__ sums, uint32_t* __restrict__ partial) {
  size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= task_off[nbuckets]) return;
  const uint2 tk = order[t];
  const size_t b = tk.x;
  const uint32_t t0 = task_off[b], nt = task_off[b + 1] - t0;
  const uint32_t off = offsets[b], cnt = offsets[b + 1] - off;
  uint32_t beg = off, end = off + cnt;
  if (nt != 1) {                                   // piece tk.y of nt equal pieces: the first cnt % nt pieces hold one entry more
    const uint32_t q = cnt / nt, r = cnt - q * nt;
    beg = off + tk.y * q + (tk.y < r ? tk.y : r); end = beg + q + (tk.y < r ? 1u : 0u);
  }
  constexpr int CW = Coord<F>::CW, XYW = 4 * CW;
  Xyzz<F> acc = xyzz_inf<F>();
  // software-pipelined gather: the next point (and the entry after it) are in flight while this one is added, so the
  // random-access latency of the table hides under ~6000 VALU instructions instead of stalling the two waves of a SIMD
  typedef typename F::E E;
  uint32_t ent = beg < end ? entries[beg] : 0, ent_next = beg + 1 < end ? entries[beg + 1] : 0;      // empty bucket: harmless load of entry 0
  const uint32_t* p = table + (size_t)(ent & 0x7fffffffu) * (2 * CW);
  E nx = Coord<F>::ld(p), ny = Coord<F>::ld(p + CW);
  for (uint32_t e = beg; e < end; ++e) {
    E x = nx, y = ny;
    const bool negate = ent >> 31;
    if (e + 1 < end) {
      ent = ent_next;
      ent_next = e + 2 < end ? entries[e + 2] : 0;
      p = table + (size_t)(ent & 0x7fffffffu) * (2 * CW);
      nx = Coord<F>::ld(p); ny = Coord<F>::ld(p + CW);
    }
    if (negate) y = F::neg(y);
    acc = xyzz_add_aff<F>(acc, x, y);
  }
  st_xy<F>(nt == 1 ? sums + b * XYW : partial + (size_t)(t0 + tk.y) * XYW, acc);
}

// ---- bucket reduction  sum_b (b+1) S_b, b = hi*NLO + lo:
//   = sum_lo (lo+1) C_lo + NLO * sum_hi hi * R_hi,   C_lo = sum_hi S, R_hi = sum_lo S
// four lanes per point operation: msm_reduce_coop.h ----
}  // namespace zkt
#include "msm_reduce_coop.h"
namespace zkt {

// direct form: total = sum_w 2^(c w) W_w.  One wave: lane w doubles its window result c*w times (the longest lane does the
// c*(nwin-1) <= 256 doublings a serial Horner would), then an LDS tree; lane 0 writes the Jacobian sum and its affine normalisation.
template <class F>
__global__ void __launch_bounds__(64) k_join_windows(const uint32_t* __restrict__ win_jac, int nwin, int c, uint32_t* __restrict__ out_jac, uint32_t* __restrict__ out_abi) {
  ZKT_SIDE_PRIO;
  constexpr int CW = Coord<F>::CW, XYW = 4 * CW, JW = 3 * CW;
  __shared__ uint32_t lds[16 * JW];
  const int t = threadIdx.x;
  auto ldj = [](const uint32_t* p) { return Jac<F>{Coord<F>::ld(p), Coord<F>::ld(p + CW), Coord<F>::ld(p + 2 * CW)}; };
  auto stj = [](uint32_t* p, const Jac<F>& a) { Coord<F>::st(p, a.X); Coord<F>::st(p + CW, a.Y); Coord<F>::st(p + 2 * CW, a.Z); };
  Jac<F> v = jac_inf<F>();
  if (t < nwin) {
    v = ldj(win_jac + (size_t)t * XYW);
    for (int d = 0; d < c * t; ++d) v = jac_dbl(v);
  }
  for (int d = 16; d >= 1; d >>= 1) {                  // nwin <= 32
    if (t >= d && t < 2 * d) stj(lds + (t - d) * JW, v);
    __syncthreads();
    if (t < d) v = jac_add(v, ldj(lds + t * JW));
    __syncthreads();
  }
  if (t == 0) {
    stj(out_jac, v);
    if (out_abi) PtIO<F>::st(out_abi, jac_to_aff(v));
  }
}

// batched form: the k sums k_combine left XYW words apart -> k Jacobian partials in the 3-coordinate layout of a single MSM's partial, and the k affine ABI points.
// One lane per vector (k <= 32): the k inversions run side by side in one wave.
template <class F>
__global__ void __launch_bounds__(64) k_batch_finish(const uint32_t* __restrict__ sum_jac, int k, uint32_t* __restrict__ out_jac, uint32_t* __restrict__ out_abi) {
  ZKT_SIDE_PRIO;
  constexpr int CW = Coord<F>::CW, XYW = 4 * CW, JW = 3 * CW;
  const int t = threadIdx.x;
  if (t >= k) return;
  const uint32_t* p = sum_jac + (size_t)t * XYW;
  const Jac<F> v{Coord<F>::ld(p), Coord<F>::ld(p + CW), Coord<F>::ld(p + 2 * CW)};
  uint32_t* o = out_jac + (size_t)t * JW;
  Coord<F>::st(o, v.X); Coord<F>::st(o + CW, v.Y); Coord<F>::st(o + 2 * CW, v.Z);
  PtIO<F>::st(out_abi + (size_t)t * PtIO<F>::WORDS, jac_to_aff(v));
}

// stage 2 (VALU bound, the dominant kernel): one bucket per lane
static hipError_t launch_accumulate(const MsmPlan& P, const uint32_t* table, void* workspace, hipStream_t s) {
  if (P.grp != GRP) return hipErrorInvalidValue;
  MsmWs w = carve(P, workspace);
#if defined(ZKT_MSM_PART_OTHER)      // G2: two lanes per task (zkt_msm_g2pair.hip); k_accumulate is not instantiated over Fq2
  return ::zkt_launch_accumulate_g2_pair(table, (const uint32_t*)w.entries, (const uint32_t*)w.offsets, (const void*)w.order, (const uint32_t*)w.task_off, P.nbuckets,
                                         w.sums, w.partial, w.max_tasks, s);
#else
  hipLaunchKernelGGL(k_accumulate<GF>, dim3(grid_blocks(w.max_tasks, 64)), dim3(64), 0, s, table, (const uint32_t*)w.entries,
                     (const uint32_t*)w.offsets, (const uint2*)w.order, (const uint32_t*)w.task_off, P.nbuckets, w.sums, w.partial);
  return hipGetLastError();
#endif
}
// stage 3 (latency bound): sum_b (b+1) S_b, b = hi*NLO + lo  ->  Jacobian partial (+ affine point if out_abi)
static hipError_t launch_reduce(const MsmPlan& P, void* workspace, uint32_t* dev_result_jac, uint32_t* dev_out_abi, hipStream_t s) {
  if (P.grp != GRP) return hipErrorInvalidValue;
  // The direct form reduces every window side by side (grid.y) and joins them, the batched form every vector and finishes them; a single resident MSM is one reduction.
  const bool many = P.direct || P.batch;
  const unsigned ny = (unsigned)(P.direct ? P.nwin : P.batch ? P.batch : 1);
  const size_t B = many ? P.half : P.nbuckets;          // buckets of one reduction
  MsmWs w = carve(P, workspace);
  const size_t NLO = B < 1024 ? B : 1024, NHI = B / NLO;
  int lo_bits = 0; while ((size_t(1) << lo_bits) < NLO) ++lo_bits;
  int hi_bits = 0; while ((size_t(1) << hi_bits) < NHI) ++hi_bits;
  const int nbA = lo_bits + 1, nbB = NHI > 1 ? hi_bits : 0;     // weights lo+1 in [1,NLO]; hi in [0,NHI)
  // pieces per row (k_marginals): a column block sums NHI points, a row piece NLO / RS — cut the rows until both carry chains of the same length
  // (at 2^16 buckets: 64 x 1024, RS = 16 gives 64-point pieces, one per lane + the tree, instead of 8 per lane), within the 1024-entry row buffer
  int RS = 1;
  while (NHI > 1 && (size_t)(2 * RS) * NHI <= 1024 && NLO / (size_t)(2 * RS) >= 64 && NLO / (size_t)(2 * RS) >= NHI) RS *= 2;
  const size_t NROW = (size_t)RS * NHI;
  const size_t merge_blocks = (P.nbuckets + RED_NG - 1) / RED_NG < 4096 ? (P.nbuckets + RED_NG - 1) / RED_NG : 4096;      // the partials of ALL buckets are merged at once
  hipLaunchKernelGGL(k_merge_hot<GF>, dim3(HOT_FAN, HOT_CAP), dim3(RED_TPB), 0, s, (const uint32_t*)w.task_off, (const uint32_t*)w.partial, (const uint32_t*)w.hot, w.hot_part);
  hipLaunchKernelGGL(k_merge_partials<GF>, dim3((unsigned)merge_blocks), dim3(RED_TPB), 0, s, (const uint32_t*)w.task_off, P.nbuckets, (const uint32_t*)w.partial, (const uint32_t*)w.hot,
                     (const uint32_t*)w.hot_part, w.sums);
  hipLaunchKernelGGL(k_marginals<GF>, dim3((unsigned)(NLO + (NHI > 1 ? NROW : 0)), ny), dim3(RED_TPB), 0, s, (const uint32_t*)w.sums, NLO, NHI, RS, w.colsum, w.rowsum);
  hipLaunchKernelGGL(k_weight_bits<GF>, dim3((unsigned)(nbA + nbB) * WB_SPLIT, ny), dim3(WB_TPB), 0, s, (const uint32_t*)w.colsum, NLO, nbA, (const uint32_t*)w.rowsum, NHI, RS, w.clsA, w.clsB);
  // one reduction: k_combine writes the result itself; many: their sums go to win_jac, XYW words apart
  hipLaunchKernelGGL(k_combine<GF>, dim3(1, ny), dim3(CMB_TPB), 0, s, (const uint32_t*)w.clsA, nbA, (const uint32_t*)w.clsB, nbB, lo_bits, many ? w.win_jac : dev_result_jac,
                     many ? (uint32_t*)nullptr : dev_out_abi);
  if (P.direct) hipLaunchKernelGGL(k_join_windows<GF>, dim3(1), dim3(64), 0, s, (const uint32_t*)w.win_jac, P.nwin, P.c, dev_result_jac, dev_out_abi);
  else if (P.batch) hipLaunchKernelGGL(k_batch_finish<GF>, dim3(1), dim3(64), 0, s, (const uint32_t*)w.win_jac, P.batch, dev_result_jac, dev_out_abi);
  return hipGetLastError();
}

// window-multiple table build
static hipError_t launch_precompute(int grp, uint32_t* table, uint8_t* inf, size_t n, int c, int nwin, uint32_t* tmp, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (grp != GRP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_precompute<GF>, dim3(grid_blocks(n, 64)), dim3(64), 0, s, table, inf, n, c, nwin, tmp);
  return hipGetLastError();
}

// combine step of a sharded MSM + affine normalisation: sum of `count` Jacobian partials (3*CW words each, `stride` words apart).
// One wave: lane t sums partials t, t+64, ..., then an LDS tree (6 levels) — 8 partials cost 3 additions of latency, not 8.
template <class F>
__global__ void __launch_bounds__(64) k_jac_sum_to_affine(const uint32_t* __restrict__ parts, size_t count, size_t stride, uint32_t* __restrict__ out_abi) {
  constexpr int CW = Coord<F>::CW, JW = 3 * CW;
  __shared__ uint32_t lds[32 * JW];
  const int t = threadIdx.x;
  auto ldj = [](const uint32_t* p) { return Jac<F>{Coord<F>::ld(p), Coord<F>::ld(p + CW), Coord<F>::ld(p + 2 * CW)}; };
  auto stj = [](uint32_t* p, const Jac<F>& a) { Coord<F>::st(p, a.X); Coord<F>::st(p + CW, a.Y); Coord<F>::st(p + 2 * CW, a.Z); };
  Jac<F> v = jac_inf<F>();
  for (size_t i = t; i < count; i += 64) v = jac_add<F>(v, ldj(parts + i * stride));
  for (int d = 32; d >= 1; d >>= 1) {
    if (t >= d && t < 2 * d) stj(lds + (t - d) * JW, v);
    __syncthreads();
    if (t < d && (size_t)(t + d) < count) v = jac_add<F>(v, ldj(lds + t * JW));
    __syncthreads();
  }
  if (t == 0) PtIO<F>::st(out_abi, jac_to_aff(v));
}
// out = a + b on Jacobian partials (3 coordinates each): two partial sums of ONE result that were accumulated over different base sets
template <class F>
__global__ void __launch_bounds__(64) k_jac_add(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  if (threadIdx.x) return;
  constexpr int CW = Coord<F>::CW;
  const Jac<F> x{Coord<F>::ld(a), Coord<F>::ld(a + CW), Coord<F>::ld(a + 2 * CW)}, y{Coord<F>::ld(b), Coord<F>::ld(b + CW), Coord<F>::ld(b + 2 * CW)};
  const Jac<F> r = jac_add<F>(x, y);
  Coord<F>::st(out, r.X); Coord<F>::st(out + CW, r.Y); Coord<F>::st(out + 2 * CW, r.Z);
}
static hipError_t launch_jac_add(int grp, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t s) {
  if (grp != GRP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_jac_add<GF>, dim3(1), dim3(64), 0, s, a, b, out);
  return hipGetLastError();
}
static hipError_t launch_jac_sum_to_affine(int grp, const uint32_t* parts, size_t count, size_t stride, uint32_t* out_abi, hipStream_t s) {
  if (grp != GRP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_jac_sum_to_affine<GF>, dim3(1), dim3(64), 0, s, parts, count, stride, out_abi);
  return hipGetLastError();
}

// what this object contributes to the pipeline: zkt_msm_dispatch.cpp holds the entry points that pick a group's table.  Host pass only: the device pass would emit a
// constant of its own, whose host function pointers nothing there defines.
#if !defined(__HIP_DEVICE_COMPILE__)
const MsmLaunchers MSM_LAUNCHERS = {launch_to_kernel_layout, launch_precompute, launch_sort, launch_sort_batch, launch_accumulate, launch_reduce, launch_jac_add, launch_jac_sum_to_affine};
#endif

}  // namespace zkt
