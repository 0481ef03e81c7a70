// Stage 1 of the MSM pipeline: signed c-bit digits, counting sort of (bucket, point) pairs by bucket, task list ordered by size.
// Nothing here depends on the group, but every zkt_msm.hip object includes it and carries its own copy, built with that object's flags: compiled once at one
// optimisation level, the G2 figures left the parent's spread (profiles/msm_sort_split_ab.md).
#pragma once
#include "msm_ws.h"

namespace zkt {

// The pipeline clears its counters with a kernel of its own rather than hipMemsetAsync: inside a captured graph (zkt_msm_handle.cpp, msm_submit) a memset becomes a
// runtime-owned node, and the pipeline's launches should be the same objects whether they are issued or replayed.
static __global__ void __launch_bounds__(256) k_zero_words(uint32_t* __restrict__ p, int head_words, size_t quads, int tail_words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)head_words) p[i] = 0u;                                              // words before the first 16-byte boundary
  uint4* q = reinterpret_cast<uint4*>(p + head_words);
  if (i < quads) q[i] = uint4{0u, 0u, 0u, 0u};
  if (i < (size_t)tail_words) p[(size_t)head_words + quads * 4 + i] = 0u;
}
// ptr 4-byte aligned (the carve puts `offsets` at 4 mod 16), bytes a multiple of 4.  (A runtime-owned memset node faults on the first replay after any later hipFree,
// zkt_msm_handle.cpp, msm_submit; a zero-term MSM is captured like any other.)
static hipError_t zero_async(void* ptr, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if (((uintptr_t)ptr & 3u) || (bytes & 3u)) return hipErrorInvalidValue;
  size_t words = bytes / 4;
  int head = (int)(((16u - ((uintptr_t)ptr & 15u)) & 15u) / 4);
  if ((size_t)head > words) head = (int)words;
  words -= (size_t)head;
  const size_t quads = words / 4; const int tail = (int)(words % 4);
  size_t items = quads > (size_t)tail ? quads : (size_t)tail;
  if (items < (size_t)head) items = (size_t)head;
  hipLaunchKernelGGL(k_zero_words, dim3(grid_blocks(items)), dim3(256), 0, s, (uint32_t*)ptr, head, quads, tail);
  return hipGetLastError();
}

// ---- signed-digit decomposition, counting sort by bucket ----
__device__ inline uint32_t window_bits(const uint32_t* k, int w, int c) {
  int o = w * c, word = o >> 5, sh = o & 31;
  if (word >= 8) return 0;
  uint64_t v = k[word];
  if (word + 1 < 8) v |= (uint64_t)k[word + 1] << 32;
  return (uint32_t)(v >> sh) & ((1u << c) - 1);
}
// |digit| in [0, 2^(c-1)] of window w of the scalar k.  neg: on entry the sign of the window below, which is the carry into this one (0 at window 0); on return this
// window's sign.  half = 2^(c-1).
__device__ inline uint32_t signed_digit(const uint32_t* k, int w, int c, uint32_t half, uint32_t& neg) {
  const uint32_t raw = window_bits(k, w, c) + neg;
  neg = raw > half;
  return neg ? (1u << c) - raw : raw;
}
__device__ inline void load_scalar(uint32_t* k /*8*/, const uint32_t* __restrict__ scalars, size_t i) {
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + i * 8);
  const uint4 lo = sp[0], hi = sp[1];
  k[0] = lo.x; k[1] = lo.y; k[2] = lo.z; k[3] = lo.w; k[4] = hi.x; k[5] = hi.y; k[6] = hi.z; k[7] = hi.w;
}

// One atomic per (scalar, window) on the bucket counter; the returned value is the entry's slot inside its bucket.  The COUNT pass keeps it
// (slot[w*n + i], a coalesced 4-byte store per window), so the SCATTER pass is atomic-free: recompute the digit, read slot and offsets[bucket],
// write the entry (13.6 M atomics at 2^20 terms were 0.5 ms of the scatter pass).
// Skewed inputs (a witness full of 0/1) send most lanes of a wave to the SAME counter, which would serialise a million
// atomics on one address: up to two rounds of wave-level aggregation elect a leader for the most common bucket id among
// the active lanes (one atomicAdd of the population count, ranks by prefix popcount); the rest go individually.
static constexpr uint32_t NO_SLOT = 0xffffffffu;          // zero digit / infinity: no entry
template <bool SCATTER>
static __global__ void __launch_bounds__(256) k_digits(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, size_t n, int c, int nwin, uint32_t win_buckets,
                                                uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                uint32_t* __restrict__ slot, uint32_t* __restrict__ entries) {
  ZKT_SIDE_PRIO;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) load_scalar(k, scalars, i);
  const uint32_t half = 1u << (c - 1);
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  uint32_t neg = 0;
  for (int w = 0; w < nwin; ++w) {                      // wave-uniform trip count: the ballots below need every lane here
    const uint32_t mag = signed_digit(k, w, c, half, neg);
    // resident form (win_buckets = 0): entry = index into the window-multiple table, one bucket set for all windows;
    // direct form: entry = the base itself, window w owns buckets [w * win_buckets, (w+1) * win_buckets)
    size_t src = win_buckets ? i : (size_t)w * n + i;
    const uint32_t b = mag - 1 + (uint32_t)w * win_buckets;
    if (SCATTER) {
      if (live) { const uint32_t pos = slot[(size_t)w * n + i]; if (pos != NO_SLOT) entries[offsets[b] + pos] = (uint32_t)src | (neg << 31); }
      continue;
    }
    bool todo = live && mag != 0 && !inf[live ? src : 0];   // infinity and zero digits contribute nothing
    uint32_t pos = NO_SLOT;
    for (int round = 0; round < 2; ++round) {
      unsigned long long act = __ballot(todo);
      if (act == 0) break;
      int leader = __ffsll((long long)act) - 1;
      uint32_t lb = __shfl(b, leader);
      unsigned long long same = __ballot(todo && b == lb);
      int cnt = __popcll(same);
      if (cnt < 4) break;                               // nothing worth aggregating: fall through to individual atomics
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&counts[lb], (uint32_t)cnt);
      base = __shfl(base, leader);
      if (todo && b == lb) { pos = base + (uint32_t)__popcll(same & lt_mask); todo = false; }
    }
    if (todo) pos = atomicAdd(&counts[b], 1u);
    if (live) slot[(size_t)w * n + i] = pos;
  }
}

// Batched form (msm_plan_batch): grid.y = scalar vector.  Vector v reads its scalars `vec_stride` scalars after vector v-1's and files its digits into bucket set v,
// buckets [v * 2^(c-1), (v+1) * 2^(c-1)); the entries still index the ONE resident window-multiple table (w * n + i, sign in bit 31), so the k bucket sets are
// accumulated by the same gather as one.  Slots are kept per (vector, window).  Zero digits, points at infinity and the wave-level aggregation are k_digits'.
template <bool SCATTER>
static __global__ void __launch_bounds__(256) k_digits_batch(const uint32_t* __restrict__ scalars, size_t vec_stride, const uint8_t* __restrict__ inf, size_t n, int c, int nwin,
                                                      uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                      uint32_t* __restrict__ slot, uint32_t* __restrict__ entries) {
  ZKT_SIDE_PRIO;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
  const bool live = i < n;
  uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) load_scalar(k, scalars, v * vec_stride + i);
  const uint32_t half = 1u << (c - 1), set = (uint32_t)v * half;
  slot += v * (size_t)nwin * n;
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  uint32_t neg = 0;
  for (int w = 0; w < nwin; ++w) {                      // wave-uniform trip count: the ballots below need every lane here
    const uint32_t mag = signed_digit(k, w, c, half, neg);
    const size_t src = (size_t)w * n + i;
    const uint32_t b = set + mag - 1;
    if (SCATTER) {
      if (live) { const uint32_t pos = slot[src]; if (pos != NO_SLOT) entries[offsets[b] + pos] = (uint32_t)src | (neg << 31); }
      continue;
    }
    bool todo = live && mag != 0 && !inf[live ? src : 0];   // infinity and zero digits contribute nothing
    uint32_t pos = NO_SLOT;
    for (int round = 0; round < 2; ++round) {
      unsigned long long act = __ballot(todo);
      if (act == 0) break;
      int leader = __ffsll((long long)act) - 1;
      uint32_t lb = __shfl(b, leader);
      unsigned long long same = __ballot(todo && b == lb);
      int cnt = __popcll(same);
      if (cnt < 4) break;                               // nothing worth aggregating: fall through to individual atomics
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&counts[lb], (uint32_t)cnt);
      base = __shfl(base, leader);
      if (todo && b == lb) { pos = base + (uint32_t)__popcll(same & lt_mask); todo = false; }
    }
    if (todo) pos = atomicAdd(&counts[b], 1u);
    if (live) slot[src] = pos;
  }
}

// exclusive scan of counts[0..m) into offsets[0..m]: per-block sums, scan of the block sums, per-block scan.
static constexpr int SCAN_TPB = 256, SCAN_ITEMS = 8;
static_assert(SCAN_TILE == SCAN_TPB * SCAN_ITEMS, "a block of the scan takes one tile");
__device__ inline uint32_t block_excl_scan_256(uint32_t v, uint32_t* lds /*256*/, uint32_t& total) {
  const int t = threadIdx.x;
  lds[t] = v; __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    uint32_t x = t >= d ? lds[t - d] : 0; __syncthreads();
    lds[t] += x; __syncthreads();
  }
  total = lds[255];
  uint32_t excl = t ? lds[t - 1] : 0;
  __syncthreads();
  return excl;
}
static __global__ void __launch_bounds__(256) k_scan_sums(const uint32_t* __restrict__ in, size_t m, uint32_t* __restrict__ blocksum) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t lds[256];
  size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < m) s += in[base + k];
  uint32_t tot; (void)block_excl_scan_256(s, lds, tot);
  if (threadIdx.x == 0) blocksum[blockIdx.x] = tot;
}
static __global__ void __launch_bounds__(256) k_scan_top(uint32_t* __restrict__ blocksum, int nblk, uint32_t* __restrict__ grand_total) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t lds[256];
  uint32_t run = 0;
  for (int base = 0; base < nblk; base += 256) {          // nblk <= 2^19/2048 = 256 in practice
    int i = base + threadIdx.x;
    uint32_t v = i < nblk ? blocksum[i] : 0, tot;
    uint32_t ex = block_excl_scan_256(v, lds, tot);
    if (i < nblk) blocksum[i] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) *grand_total = run;
}
static __global__ void __launch_bounds__(256) k_scan_final(const uint32_t* __restrict__ in, size_t m, const uint32_t* __restrict__ blocksum,
                                                    uint32_t* __restrict__ out) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t lds[256];
  size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = base + k < m ? in[base + k] : 0; s += v[k]; }
  uint32_t tot; uint32_t run = block_excl_scan_256(s, lds, tot) + blocksum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) { if (base + k < m) out[base + k] = run; run += v[k]; }
}
// (Round 4 measured ONE block scanning a small set's counters — and the task count fused into that scan — to save kernel nodes of a small MSM's graph: the one-block scan of
//  65,536 counters takes 40 us against 18 us for the three kernels below plus their launch gaps, and the 2^17-term MSM, the range proof and the small Groth16 keys did not move
//  (1.28 ms, 3.3-3.6 ms, 2.5 ms).  Taken out again: a node of a replayed graph does not cost what DESIGN §9 (round 3) assumed.)
// out[0..m) = exclusive scan of in, out[m] = total.  scratch: >= ceil(m/2048) words
static void launch_scan(const uint32_t* in, uint32_t* out, size_t m, uint32_t* scratch, hipStream_t s) {
  int nblk = (int)((m + SCAN_TILE - 1) / SCAN_TILE);
  hipLaunchKernelGGL(k_scan_sums, dim3(nblk), dim3(256), 0, s, in, m, scratch);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, s, scratch, nblk, out + m);
  hipLaunchKernelGGL(k_scan_final, dim3(nblk), dim3(256), 0, s, in, m, (const uint32_t*)scratch, out);
}

// ---- counting sort by bucket WITHOUT global atomics (large MSMs): two-level radix partition through LDS histograms ----
// k_digits pays one returning global atomic per (scalar, window) — 13.6 M of them at 2^20 terms, executed at the memory side at ~25 G/s whatever the
// occupancy: 0.55 ms for the count pass plus 0.22-0.35 ms for the scatter, and two sorts side by side in a Groth16 proof slow each other to 1.9 + 2.6 ms.
// Here the bucket id is split into a partition (its high bits) and a position inside the partition (its low PART_LO bits):
//   pass A  every tile of PART_TILE scalars (4 per thread of a 256-thread block: 1,024 blocks at 2^20 terms — with 16 per thread the pass had one block per CU and took
//           140 us instead of 57; a block small enough to find room beside the accumulate waves of a neighbouring MSM — 1024-thread blocks waited 1.8 ms for a
//           free CU in the pipeline) histograms its digits by PARTITION in LDS                 -> tilehist[partition][tile]
//   scan    (partition-major) gives every (partition, tile) its segment of the record array
//   pass B  the tiles recompute their digits and write (entry, low bits) records into their segments     (ranks from LDS atomics; ONE 8-byte store per record:
//           the pass is bound by the NUMBER of scattered stores — 316 us with a 4-byte and a 2-byte store per record, 180 us with one)
//   pass C  every partition is cut into chunks of PART_CHUNK records; a block histograms the low bits of its chunk in LDS (C1), one block per partition
//           turns the chunk histograms into running offsets and the bucket totals into counts[] / offsets[] (C1b), and the chunk blocks place their
//           entries (C2).  A skewed input (a witness of 0/1: a million entries in one partition) is simply more chunks.
// (Round 3 also measured both scatter passes with their runs staged through LDS — records grouped by partition / bucket in a 48-56 KB stage and written out in order, to
//  cure the 7x write amplification the counters show (592 + 369 MB written for 82 + 54 MB of payload).  Pass C2 took the same 165 us staged as direct, pass B 893 us
//  instead of 313 (its 4096-scalar tile only fits the stage in eight partition ranges, each re-deriving the digits): the partial-sector writes are absorbed by the memory
//  side, the passes are bound by their LDS atomics and latency.  Taken out again.)
// Every pass streams: ~310 MB at 2^20 terms instead of 13.6 M scattered read-modify-writes.  counts / offsets / entries come out exactly as from k_digits
// (the order of the entries inside a bucket is arbitrary in both), so everything downstream is unchanged.
template <bool SCATTER>
static __global__ void __launch_bounds__(PART_TPB) k_part_tiles(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, size_t n, int c, int nwin, uint32_t win_buckets,
                                                    uint32_t P, uint32_t ntiles, uint32_t* __restrict__ tilehist, const uint32_t* __restrict__ tileoff,
                                                    uint2* __restrict__ rec) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t h[PART_MAXP];
  for (uint32_t p = threadIdx.x; p < P; p += PART_TPB) h[p] = SCATTER ? tileoff[(size_t)p * ntiles + blockIdx.x] : 0u;
  __syncthreads();
  const uint32_t half = 1u << (c - 1);
  // two scalars per trip: their loads, and the LDS atomic -> store chains of their digits, are in flight together (one scalar at a time the pass is a latency chain)
  for (int j = 0; j < PART_TILE / PART_TPB; j += 2) {
    const size_t i0 = (size_t)blockIdx.x * PART_TILE + j * PART_TPB + threadIdx.x, i1 = i0 + PART_TPB;
    const bool v0 = i0 < n, v1 = i1 < n;
    uint32_t k0[8] = {}, k1[8] = {};
    if (v0) load_scalar(k0, scalars, i0);
    if (v1) load_scalar(k1, scalars, i1);
    uint32_t carry0 = 0, carry1 = 0;
    for (int w = 0; w < nwin; ++w) {
      // (not signed_digit: two calls in a row order the six operations scalar by scalar, and the compiler then schedules the loop differently)
      const uint32_t raw0 = window_bits(k0, w, c) + carry0, raw1 = window_bits(k1, w, c) + carry1;
      const uint32_t neg0 = raw0 > half, neg1 = raw1 > half;
      const uint32_t mag0 = neg0 ? (1u << c) - raw0 : raw0, mag1 = neg1 ? (1u << c) - raw1 : raw1;
      carry0 = neg0; carry1 = neg1;
      const size_t src0 = win_buckets ? i0 : (size_t)w * n + i0, src1 = win_buckets ? i1 : (size_t)w * n + i1;
      const bool a0 = v0 && mag0 != 0 && !inf[src0], a1 = v1 && mag1 != 0 && !inf[src1];       // infinity and zero digits contribute nothing
      const uint32_t b0 = mag0 - 1 + (uint32_t)w * win_buckets, b1 = mag1 - 1 + (uint32_t)w * win_buckets;
      uint32_t pos0 = 0, pos1 = 0;
      if (a0) pos0 = atomicAdd(&h[b0 >> PART_LO], 1u);
      if (a1) pos1 = atomicAdd(&h[b1 >> PART_LO], 1u);
      if (SCATTER) {
        // ONE 8-byte store per record (entry, low bits): the pass is bound by the number of scattered stores, not by their bytes (two stores per record: 285 us)
        if (a0) rec[pos0] = make_uint2((uint32_t)src0 | (neg0 << 31), b0 & (PART_SUB - 1));
        if (a1) rec[pos1] = make_uint2((uint32_t)src1 | (neg1 << 31), b1 & (PART_SUB - 1));
      }
    }
  }
  if (!SCATTER) {
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < P; p += PART_TPB) tilehist[(size_t)p * ntiles + blockIdx.x] = h[p];
  }
}
// chunk blocks of every partition: blkoff[p] = first block of partition p, blkoff[P] = blocks in use (one block: P <= PART_MAXP)
static __global__ void __launch_bounds__(256) k_part_blocks(const uint32_t* __restrict__ tileoff, uint32_t P, uint32_t ntiles, uint32_t* __restrict__ blkoff) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t lds[256];
  constexpr int ITEMS = PART_MAXP / 256;
  uint32_t v[ITEMS], sum = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const uint32_t p = threadIdx.x * ITEMS + k;
    uint32_t cnt = 0;
    if (p < P) { const uint32_t size = tileoff[(size_t)(p + 1) * ntiles] - tileoff[(size_t)p * ntiles]; cnt = (size + PART_CHUNK - 1) / PART_CHUNK; }
    v[k] = cnt; sum += cnt;
  }
  uint32_t tot; uint32_t run = block_excl_scan_256(sum, lds, tot);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) { const uint32_t p = threadIdx.x * ITEMS + k; if (p < P) blkoff[p] = run; run += v[k]; }
  if (threadIdx.x == 0) blkoff[P] = tot;
}
// which (partition, chunk) block `blk` is: the last p with blkoff[p] <= blk
__device__ inline uint32_t part_of_block(const uint32_t* __restrict__ blkoff, uint32_t P, uint32_t blk) {
  uint32_t lo = 0, hi = P;                          // invariant: blkoff[lo] <= blk < blkoff[hi]
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (blkoff[mid] <= blk) lo = mid; else hi = mid; }
  return lo;
}
template <bool PLACE>
static __global__ void __launch_bounds__(256) k_part_chunks(const uint32_t* __restrict__ tileoff, uint32_t P, uint32_t ntiles, const uint32_t* __restrict__ blkoff,
                                                     const uint2* __restrict__ rec, uint32_t* __restrict__ subhist,
                                                     const uint32_t* __restrict__ offsets, size_t nbuckets, uint32_t* __restrict__ entries) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t h[PART_SUB];
  const uint32_t blk = blockIdx.x;
  if (blk >= blkoff[P]) return;                     // block-uniform
  const uint32_t p = part_of_block(blkoff, P, blk), chunk = blk - blkoff[p];
  const uint32_t pbeg = tileoff[(size_t)p * ntiles], pend = tileoff[(size_t)(p + 1) * ntiles];
  const uint32_t beg = pbeg + chunk * PART_CHUNK, end = beg + PART_CHUNK < pend ? beg + PART_CHUNK : pend;
  for (int t = threadIdx.x; t < PART_SUB; t += 256) {
    const size_t b = (size_t)p * PART_SUB + t;
    h[t] = PLACE ? (b < nbuckets ? offsets[b] + subhist[(size_t)blk * PART_SUB + t] : 0u) : 0u;
  }
  __syncthreads();
  // four records per lane and trip: the loads of a trip are in flight together (the loop is a chain of load -> LDS atomic -> store otherwise: 165 us for 136 MB)
  uint32_t r = beg + threadIdx.x;
  for (; r + 3 * 256 < end; r += 4 * 256) {
    const uint2 r0 = rec[r], r1 = rec[r + 256], r2 = rec[r + 512], r3 = rec[r + 768];
    const uint32_t p0 = atomicAdd(&h[r0.y], 1u), p1 = atomicAdd(&h[r1.y], 1u), p2 = atomicAdd(&h[r2.y], 1u), p3 = atomicAdd(&h[r3.y], 1u);
    if (PLACE) { entries[p0] = r0.x; entries[p1] = r1.x; entries[p2] = r2.x; entries[p3] = r3.x; }
  }
  for (; r < end; r += 256) {
    const uint2 rr = rec[r];
    const uint32_t pos = atomicAdd(&h[rr.y], 1u);
    if (PLACE) entries[pos] = rr.x;
  }
  if (!PLACE) {
    __syncthreads();
    for (int t = threadIdx.x; t < PART_SUB; t += 256) subhist[(size_t)blk * PART_SUB + t] = h[t];
  }
}
// one block per partition: chunk histograms -> running offsets (in place); bucket totals -> counts[], offsets[] (and offsets[nbuckets] = all entries)
static __global__ void __launch_bounds__(PART_SUB) k_part_offsets(const uint32_t* __restrict__ tileoff, uint32_t P, uint32_t ntiles, const uint32_t* __restrict__ blkoff,
                                                           uint32_t* __restrict__ subhist, size_t nbuckets, uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t sc[PART_SUB];
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  uint32_t run = 0;
  for (uint32_t cblk = blkoff[p]; cblk < blkoff[p + 1]; ++cblk) { const uint32_t v = subhist[(size_t)cblk * PART_SUB + t]; subhist[(size_t)cblk * PART_SUB + t] = run; run += v; }
  sc[t] = run; __syncthreads();
  for (int d = 1; d < PART_SUB; d <<= 1) { const uint32_t x = t >= (uint32_t)d ? sc[t - d] : 0u; __syncthreads(); sc[t] += x; __syncthreads(); }
  const size_t b = (size_t)p * PART_SUB + t;
  if (b < nbuckets) { counts[b] = run; offsets[b] = tileoff[(size_t)p * ntiles] + sc[t] - run; }
  if (p == P - 1 && t == 0) offsets[nbuckets] = tileoff[(size_t)P * ntiles];
}

// Work list.  A bucket of cnt entries is cut into nt = ceil(cnt / chunk) equal pieces (the first cnt % nt of them one entry longer), one
// piece per lane ("task"), so one lane never runs an unbounded list: with random scalars at 2^20 terms every bucket (~26 entries) is a single
// task, while skewed inputs (many equal scalars: a real witness is full of 0/1) and small MSMs (chunk from pick_chunk) spread their buckets
// over many lanes, whose partial sums are merged afterwards.  Tasks are ordered by size (largest first) by a counting sort, so the 64 lanes
// of a wave run equally long lists.  (CHUNK, SIZE_BINS and the HOT_* limits: msm_ws.h)
__device__ inline uint32_t ntasks_of(uint32_t c, uint32_t chunk) { return c <= chunk ? 1u : (c + chunk - 1) / chunk; }
__device__ inline uint32_t task_size_of(uint32_t c, uint32_t nt) { return (c + nt - 1) / nt; }      // the larger of the two piece sizes
static __global__ void __launch_bounds__(256) k_task_count(const uint32_t* __restrict__ counts, size_t m, uint32_t chunk, uint32_t* __restrict__ ntask, uint32_t* __restrict__ hist) {
  ZKT_SIDE_PRIO;
  __shared__ uint32_t h[SIZE_BINS];
  for (int i = threadIdx.x; i < SIZE_BINS; i += 256) h[i] = 0;
  __syncthreads();
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) {
    uint32_t c = counts[i], nt = ntasks_of(c, chunk);
    ntask[i] = nt;
    atomicAdd(&h[CHUNK - task_size_of(c, nt)], nt);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SIZE_BINS; k += 256) if (h[k]) atomicAdd(&hist[k], h[k]);
}
static __global__ void __launch_bounds__(256) k_task_scatter(const uint32_t* __restrict__ counts, size_t m, uint32_t chunk, const uint32_t* __restrict__ size_hist,
                                                      uint32_t* __restrict__ bincur, uint2* __restrict__ order, uint32_t* __restrict__ hot) {
  ZKT_SIDE_PRIO;
  // rank inside the block with LDS atomics, then ONE global atomic per (block, non-empty bin): ~50 distinct sizes
  // are shared by 2^19 buckets, so per-element global atomics would serialise.  The exclusive scan of the SIZE_BINS-entry
  // histogram (bin offsets in the size-ordered task list) is recomputed by every block: 129 values, cheaper than three more launches.
  __shared__ uint32_t h[SIZE_BINS], base[SIZE_BINS], binoff[SIZE_BINS + 1], scan[256];
  __shared__ uint32_t hot_n, hot_b[256], hot_pos[256], hot_nt[256];
  for (int i = threadIdx.x; i < SIZE_BINS; i += 256) h[i] = 0;
  if (threadIdx.x == 0) hot_n = 0;
  {
    static_assert(SIZE_BINS <= 256, "one histogram bin per thread");
    uint32_t v = threadIdx.x < SIZE_BINS ? size_hist[threadIdx.x] : 0, tot;
    uint32_t ex = block_excl_scan_256(v, scan, tot);
    if (threadIdx.x < SIZE_BINS) binoff[threadIdx.x] = ex;
  }
  __syncthreads();
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bin = 0, rank = 0, nt = 1;
  if (i < m) { uint32_t c = counts[i]; nt = ntasks_of(c, chunk); bin = CHUNK - task_size_of(c, nt); rank = atomicAdd(&h[bin], nt); }
  __syncthreads();
  for (int k = threadIdx.x; k < SIZE_BINS; k += 256) if (h[k]) base[k] = binoff[k] + atomicAdd(&bincur[k], h[k]);
  __syncthreads();
  if (i < m) {
    const uint32_t pos = base[bin] + rank;
    if (nt <= 16) { for (uint32_t k = 0; k < nt; ++k) order[pos + k] = make_uint2((uint32_t)i, k); }
    else { const uint32_t slot = atomicAdd(&hot_n, 1u); hot_b[slot] = (uint32_t)i; hot_pos[slot] = pos; hot_nt[slot] = nt; }      // a hot bucket: the whole block writes its tasks
    if (nt > HOT_NT) { const uint32_t g = atomicAdd(&hot[0], 1u); if (g < HOT_CAP) hot[1 + g] = (uint32_t)i; }
  }
  __syncthreads();
  for (uint32_t hb = 0; hb < hot_n; ++hb) {
    const uint32_t b = hot_b[hb], pos = hot_pos[hb], cnt = hot_nt[hb];
    for (uint32_t k = threadIdx.x; k < cnt; k += 256) order[pos + k] = make_uint2(b, k);
  }
}
// the tail of both sorts: tasks per bucket, their offsets, the size-ordered task list and the hot list
static hipError_t launch_task_list(const MsmPlan& P, const MsmWs& w, hipStream_t s) {
  const size_t B = P.nbuckets;
  hipLaunchKernelGGL(k_task_count, dim3(grid_blocks(B)), dim3(256), 0, s, w.counts, B, P.chunk, w.ntask, w.size_hist);
  launch_scan(w.ntask, w.task_off, B, w.scan_tmp, s);
  hipLaunchKernelGGL(k_task_scatter, dim3(grid_blocks(B)), dim3(256), 0, s, w.counts, B, P.chunk, (const uint32_t*)w.size_hist, w.size_cur, w.order, w.hot);
  return hipGetLastError();
}

// stage 1 (atomic/memory bound): signed digits, counting sort by bucket, bucket order by population
static hipError_t launch_sort(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, void* workspace, hipStream_t s) {
  const size_t B = P.nbuckets, n = P.n;
  MsmWs w = carve(P, workspace);
  hipError_t e;
  if ((e = zero_async(w.zero_begin, (uint8_t*)w.zero_end - (uint8_t*)w.zero_begin, s)) != hipSuccess) return e;
  const PartDims pd = part_dims(n, B, P.nwin);
  const bool partition = (size_t)P.nwin * n >= (size_t(1) << 22);        // below ~2^18 terms the atomics are as fast and take fewer launches
  const uint32_t wb = P.direct ? (uint32_t)P.half : 0u;
  if (n && partition && pd.P <= PART_MAXP) {
    // large MSMs: the atomic-free two-level partition (k_part_*)
    hipLaunchKernelGGL(k_part_tiles<false>, dim3(pd.ntiles), dim3(PART_TPB), 0, s, scalars, inf, n, P.c, P.nwin, wb, pd.P, pd.ntiles, w.tilehist, (const uint32_t*)nullptr, (uint2*)nullptr);
    launch_scan(w.tilehist, w.tileoff, (size_t)pd.P * pd.ntiles, w.part_scan, s);
    hipLaunchKernelGGL(k_part_tiles<true>, dim3(pd.ntiles), dim3(PART_TPB), 0, s, scalars, inf, n, P.c, P.nwin, wb, pd.P, pd.ntiles, (uint32_t*)nullptr, (const uint32_t*)w.tileoff, w.rec);
    hipLaunchKernelGGL(k_part_blocks, dim3(1), dim3(256), 0, s, (const uint32_t*)w.tileoff, pd.P, pd.ntiles, w.blkoff);
    hipLaunchKernelGGL(k_part_chunks<false>, dim3(pd.maxblk), dim3(256), 0, s, (const uint32_t*)w.tileoff, pd.P, pd.ntiles, (const uint32_t*)w.blkoff, (const uint2*)w.rec,
                       w.subhist, (const uint32_t*)nullptr, B, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_part_offsets, dim3(pd.P), dim3(PART_SUB), 0, s, (const uint32_t*)w.tileoff, pd.P, pd.ntiles, (const uint32_t*)w.blkoff, w.subhist, B, w.counts, w.offsets);
    hipLaunchKernelGGL(k_part_chunks<true>, dim3(pd.maxblk), dim3(256), 0, s, (const uint32_t*)w.tileoff, pd.P, pd.ntiles, (const uint32_t*)w.blkoff, (const uint2*)w.rec,
                       w.subhist, (const uint32_t*)w.offsets, B, w.entries);
  } else if (n) {
    const unsigned g = grid_blocks(n);
    hipLaunchKernelGGL(k_digits<false>, dim3(g), dim3(256), 0, s, scalars, inf, n, P.c, P.nwin, wb, w.counts, (const uint32_t*)nullptr, w.slot, (uint32_t*)nullptr);
    launch_scan(w.counts, w.offsets, B, w.scan_tmp, s);
    hipLaunchKernelGGL(k_digits<true>, dim3(g), dim3(256), 0, s, scalars, inf, n, P.c, P.nwin, wb, (uint32_t*)nullptr, (const uint32_t*)w.offsets, w.slot, w.entries);
  } else if ((e = zero_async(w.offsets, (B + 1) * 4, s)) != hipSuccess) return e;
  return launch_task_list(P, w, s);
}
// the same stage for a batch (P.batch vectors, `vec_stride` scalars apart): one digit pass over (vector, term), then the task list over all P.batch bucket sets
static hipError_t launch_sort_batch(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, size_t vec_stride, void* workspace, hipStream_t s) {
  const size_t B = P.nbuckets, n = P.n;
  if (P.batch < 1 || P.direct || vec_stride < n || B > (size_t)1024 * SCAN_TILE) return hipErrorInvalidValue;      // (launch_scan's scratch: 1024 block sums)
  MsmWs w = carve(P, workspace);
  hipError_t e;
  if ((e = zero_async(w.zero_begin, (uint8_t*)w.zero_end - (uint8_t*)w.zero_begin, s)) != hipSuccess) return e;
  if (n) {
    const dim3 g(grid_blocks(n), (unsigned)P.batch);
    hipLaunchKernelGGL(k_digits_batch<false>, g, dim3(256), 0, s, scalars, vec_stride, inf, n, P.c, P.nwin, w.counts, (const uint32_t*)nullptr, w.slot, (uint32_t*)nullptr);
    launch_scan(w.counts, w.offsets, B, w.scan_tmp, s);
    hipLaunchKernelGGL(k_digits_batch<true>, g, dim3(256), 0, s, scalars, vec_stride, inf, n, P.c, P.nwin, (uint32_t*)nullptr, (const uint32_t*)w.offsets, w.slot, w.entries);
  } else if ((e = zero_async(w.offsets, (B + 1) * 4, s)) != hipSuccess) return e;
  return launch_task_list(P, w, s);
}

}  // namespace zkt
