// The MSM's plans and the carve-up of its workspace: host code only, also part of the test-only host build (hostcheck.cpp), where
// tests/test_msm_plan_model.py holds every plan's ws_bytes against what the carve hands out.
#include <cstdlib>
#include "msm_ws.h"

namespace zkt {

PartDims part_dims(size_t n, size_t nbuckets, int nwin) {
  PartDims d; d.P = (uint32_t)((nbuckets + PART_SUB - 1) / PART_SUB); d.ntiles = (uint32_t)((n + PART_TILE - 1) / PART_TILE);
  d.maxblk = d.P + (uint32_t)((size_t)nwin * n / PART_CHUNK) + 1; return d;
}
size_t part_ws_bytes(size_t n, size_t nbuckets, int nwin) {
  const PartDims d = part_dims(n, nbuckets, nwin);
  return 1024 + (size_t)nwin * n * 8 + 256 + 2 * ((size_t)d.P * d.ntiles + 1) * 4 + ((size_t)d.P + 1) * 4 + ((size_t)d.P * d.ntiles / 2048 + 2) * 4 + 256 + (size_t)d.maxblk * PART_SUB * 4;
}

// Task granularity (entries per lane-task of the accumulate kernel) as a function of the problem: large MSMs keep long chains (128: the
// partial sums of split buckets cost a full addition each), small ones are cut until the grid fills the chip — at 2^17 terms a chunk of 128
// left 65,536 one-bucket tasks = ONE wave per SIMD, each lane a serial chain of 32-55 additions at the single-wave multiply-add rate
// (1.37 ms for an eighth of the work of a 2^20-term MSM, profiles/r02_msm_latency_kernel_trace.txt).
uint32_t pick_chunk(size_t entries, int grp) {
  // lanes to fill: 256 CUs x 4 SIMDs x 2 waves x 64 lanes (G1, secp256k1), x 1.5 so that the short tail tasks have something to hide under;
  // the G2 pair kernel runs one wave per SIMD and two lanes per task
  const size_t tasks = grp == G_G2 ? (size_t)65536 : (size_t)196608;
  size_t c = (entries + tasks - 1) / tasks;
  if (c < 8) c = 8;
  if (c > CHUNK) c = CHUNK;
  return (uint32_t)c;
}

MsmPlan msm_plan(size_t n, int grp) {
  MsmPlan p; p.n = n; p.grp = grp;
  const size_t XYW = 4 * (size_t)coord_words(grp);
  int lg = 0; while ((size_t(1) << (lg + 1)) <= (n ? n : 1)) ++lg;   // floor(log2 n)
  // Window width.  2^20 terms: c = 20, 2^19 buckets ~ n/2, ~2*nwin ~ 26 points per bucket.  Below 2^19 terms the MSM is latency-bound and the width is MEASURED, not derived
  // (profiles/r04_msm_window_sweep.txt: single and pipelined time of resident G1 and G2 MSMs over widths and sizes 2^4 .. 2^19).  Round 3's c = floor(log2 n) met widths whose
  // TOP window holds a few bits of a 255-bit scalar (256 + c is not a multiple of c: the last window is a remainder; three bits at c = 12, 14, 18): every scalar then lands in one
  // of 8-16 NEIGHBOURING buckets of that window, which (i) one tile of k_merge_partials summed one after the other (0.84 ms of a 1.6 ms MSM at 2^14 terms — fixed there: tiles
  // are strided now) and (ii) serialise the counting sort's atomics on 8-16 counters (k_digits 1.2-1.5 ms at 2^18 terms, c = 18).  The plan picks widths that measured well on
  // both counts: 16 from 2^14 terms on (windows end exactly at bit 256: no remainder window), 13 / 11 / 10 below.  c = 17 -> 16 at 2^17 terms: 1.24 -> 1.14 ms single,
  // 2^18 terms 2.90 -> 1.62 ms, G2 at 2^18 terms 6.2 -> 4.2 ms, a rank's share of a sharded Groth16 proof 6.3 -> 5.1 ms; 2^19 terms: c = 20 as well (2.17 / 1.45 ms single /
  // pipelined against 3.27 / 1.69 at c = 19).
  static const int forced_c = [] { const char* e = getenv("ZKT_MSM_C"); return e ? atoi(e) : 0; }();
  int c = lg >= 19 ? 20 : lg >= 14 ? 16 : lg >= 11 ? 13 : lg == 10 ? 11 : 10;      // (2^19 terms: c = 20 as well — 2.17 / 1.45 ms single / pipelined against 3.27 / 1.69 at c = 19)
  if (forced_c) c = forced_c;
  if (c < 4) c = 4;
  if (c > 20) c = 20;
  p.c = c; p.nwin = (256 + 1 + c - 1) / c; p.nbuckets = size_t(1) << (c - 1);
  size_t ent = (size_t)p.nwin * n;
  p.chunk = pick_chunk(ent, grp);
  // restates what carve() hands out, with slack at its end (public through zkt_g1_msm_workspace_bytes; tests/test_msm_plan_model.py holds the carve's end against it)
  size_t b = 0;
  b += (p.nbuckets + 1) * 4 * 3;          // counts, offsets, cursor
  b += 2 * ent * 4 + 256;                  // entries, slots
  b += p.nbuckets * XYW * 4;               // bucket sums
  b += (2048 + 64 * 4) * XYW * 4;          // row/col sums, bit classes (WB_SPLIT = 4 parts each)
  b += (1024 + 3 * 1025) * 4 + 2 * (p.nbuckets + 1) * 4;          // scan scratch, size bins, task counts/offsets
  b += (p.nbuckets + ent / p.chunk + 2) * (8 + XYW * 4);          // task list + partial sums of split buckets
  b += 64 * 64 * XYW * 4 + 1024;                                  // block sums of hot buckets (k_merge_hot), hot list
  b += part_ws_bytes(n, p.nbuckets, p.nwin);
  b += 4096;
  p.ws_bytes = b;
  p.direct = 0; p.half = p.nbuckets;
  return p;
}
MsmPlan msm_plan_direct(size_t n, int grp) {
  MsmPlan p; p.n = n; p.grp = grp;
  const size_t XYW = 4 * (size_t)coord_words(grp);
  int lg = 0; while ((size_t(1) << (lg + 1)) <= (n ? n : 1)) ++lg;
  int c = lg - 3;                   // every window has its own buckets: fewer, fuller buckets than the shared form
  if (c < 9) c = 9;                 // nwin <= 29: k_join_windows folds at most 32 windows in one wave
  if (c > 16) c = 16;
  p.c = c; p.nwin = (256 + 1 + c - 1) / c; p.half = size_t(1) << (c - 1); p.nbuckets = (size_t)p.nwin * p.half; p.direct = 1;
  size_t ent = (size_t)p.nwin * n;
  p.chunk = pick_chunk(ent, grp);
  size_t b = 0;
  b += (p.nbuckets + 1) * 4 * 3 + 2 * ent * 4 + 256 + p.nbuckets * XYW * 4;
  b += (size_t)p.nwin * (2048 + 64 * 4 + 1) * XYW * 4;           // per-window row/col sums, bit classes (4 parts each), window results
  b += (1024 + 3 * 1025) * 4 + 2 * (p.nbuckets + 1) * 4;
  b += (p.nbuckets + ent / p.chunk + 2) * (8 + XYW * 4);
  b += 64 * 64 * XYW * 4 + 1024;
  b += part_ws_bytes(n, p.nbuckets, p.nwin);
  b += 8192;
  p.ws_bytes = b;
  return p;
}
// Batched form: k scalar vectors over ONE resident base set.  The handle's table was built for msm_plan's c / nwin, so the width is that plan's; vector v owns
// bucket set v (2^(c-1) buckets each, k sets side by side in one workspace), and the task granularity is picked over all k * nwin * n digits: the point of the form
// is that k latency-bound slivers become one grid.  The workspace is what the carve hands out for this plan (no partition-sort scratch).
MsmPlan msm_plan_batch(size_t n, int grp, int k) {
  MsmPlan p = msm_plan(n, grp);
  p.batch = k; p.half = size_t(1) << (p.c - 1); p.nbuckets = (size_t)k * p.half;
  p.chunk = pick_chunk((size_t)k * p.nwin * n, grp);
  p.ws_bytes = (size_t)(carve(p, nullptr).end - (uint8_t*)nullptr) + 4096;
  return p;
}

MsmWs carve(const MsmPlan& P, void* workspace) {
  const size_t B = P.nbuckets, XYW = 4 * (size_t)coord_words(P.grp);
  const size_t ent = (size_t)P.nwin * P.n * (P.batch ? (size_t)P.batch : 1);      // (vector, window, term) digits of a batch
  uint8_t* ws = (uint8_t*)workspace;
  MsmWs w;
  w.zero_begin = (uint32_t*)ws;
  w.counts = (uint32_t*)ws; ws += (B + 1) * 4;
  w.cursor = (uint32_t*)ws; ws += (B + 1) * 4;
  w.size_hist = (uint32_t*)ws; ws += (SIZE_BINS + 1) * 4;
  w.size_off = (uint32_t*)ws; ws += (SIZE_BINS + 1) * 4;
  w.size_cur = (uint32_t*)ws; ws += (SIZE_BINS + 1) * 4;
  w.hot = (uint32_t*)ws; ws += (HOT_CAP + 1) * 4;
  w.zero_end = (uint32_t*)ws;
  w.offsets = (uint32_t*)ws; ws += (B + 1) * 4;
  ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  w.entries = (uint32_t*)ws; ws += ent * 4;
  ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  w.slot = (uint32_t*)ws; ws += ent * 4;
  ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  w.sums = (uint32_t*)ws; ws += B * XYW * 4;
  const size_t nw = P.direct ? (size_t)P.nwin : P.batch ? (size_t)P.batch : 1;      // the direct form reduces every window side by side, the batched form every vector
  w.colsum = (uint32_t*)ws; ws += nw * 1024 * XYW * 4;
  w.rowsum = (uint32_t*)ws; ws += nw * 1024 * XYW * 4;
  w.clsA = (uint32_t*)ws; ws += nw * 32 * WB_SPLIT * XYW * 4;
  w.clsB = (uint32_t*)ws; ws += nw * 32 * WB_SPLIT * XYW * 4;
  w.win_jac = (uint32_t*)ws; ws += nw * XYW * 4;
  w.scan_tmp = (uint32_t*)ws; ws += 1024 * 4;
  w.ntask = (uint32_t*)ws; ws += (B + 1) * 4;
  w.task_off = (uint32_t*)ws; ws += (B + 1) * 4;
  w.max_tasks = B + ent / P.chunk + 1;
  ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  w.order = (uint2*)ws; ws += w.max_tasks * 8;
  w.partial = (uint32_t*)ws; ws += w.max_tasks * XYW * 4;
  w.hot_part = (uint32_t*)ws; ws += (size_t)HOT_CAP * HOT_FAN * XYW * 4;
  w.rec = nullptr; w.tilehist = w.tileoff = w.blkoff = w.part_scan = w.subhist = nullptr;
  if (!P.batch) {                                                  // the batched sort is k_digits_batch at every size: no partition scratch
    const PartDims d = part_dims(P.n, P.nbuckets, P.nwin);
    ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    w.rec = (uint2*)ws; ws += (((size_t)P.nwin * P.n * 8) + 255) & ~(size_t)255;
    w.tilehist = (uint32_t*)ws; ws += ((size_t)d.P * d.ntiles + 1) * 4;
    w.tileoff = (uint32_t*)ws; ws += ((size_t)d.P * d.ntiles + 1) * 4;
    w.blkoff = (uint32_t*)ws; ws += ((size_t)d.P + 1) * 4;
    w.part_scan = (uint32_t*)ws; ws += ((size_t)d.P * d.ntiles / 2048 + 2) * 4;
    ws = (uint8_t*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    w.subhist = (uint32_t*)ws; ws += (size_t)d.maxblk * PART_SUB * 4;
  }
  w.end = ws;
  return w;
}

}  // namespace zkt
