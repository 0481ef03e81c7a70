// The two per-key device caches of the Groth16 verifier (groth16_vk_cache.h).  Host code only: streams, events and the launch_* functions of zkt_internal.h.
#include <vector>
#include <mutex>
#include <cstring>
#include "host_abi.h"
#include "groth16_vk_cache.h"

namespace zkt {
// Fixed-base tables of a verifying key's statement points (launch_fixed_tables: 64 multiples 16^w P per point, ~3 ms to build), kept for the last few
// keys seen: a verifier checks many proofs against ONE key, and with the tables the statement sum of a proof is one short launch instead of a 255-step
// scalar multiplication per wire (4 of the 9 ms of a single verification).  Keyed by the points' bytes; device memory is released with the entry.
struct StmtTables { std::vector<uint8_t> key; std::shared_ptr<void> tables; uint64_t stamp = 0; };
static std::mutex g_stmt_mu; static StmtTables g_stmt[4]; static uint64_t g_stmt_clock = 0;
std::shared_ptr<void> stmt_tables_for(const zkt_g1_affine* pts, size_t n_stmt, const uint32_t* dU, hipStream_t s) {
  if (n_stmt < 1 || n_stmt > 12) return nullptr;
  const size_t kb = n_stmt * G1B;
  std::lock_guard<std::mutex> lk(g_stmt_mu);
  StmtTables* victim = &g_stmt[0];
  for (StmtTables& e : g_stmt) {
    if (e.tables && e.key.size() == kb && memcmp(e.key.data(), pts, kb) == 0) { e.stamp = ++g_stmt_clock; return e.tables; }
    if (e.stamp < victim->stamp) victim = &e;
  }
  void* mem = nullptr;
  if (hipMalloc(&mem, n_stmt * 64 * G1B) != hipSuccess) return nullptr;
  std::shared_ptr<void> t(mem, [](void* q) { if (q) hipFree(q); });
  FixedTables ft{}; ft.n = (int)n_stmt;
  for (size_t j = 0; j < n_stmt; ++j) { ft.point[j] = dU + j * (G1B / 4); ft.table[j] = (uint32_t*)mem + j * 64 * (G1B / 4); }
  if (launch_fixed_tables(G_G1, ft, s) != hipSuccess) return nullptr;
  victim->tables = t; victim->key.assign((const uint8_t*)pts, (const uint8_t*)pts + kb); victim->stamp = ++g_stmt_clock;
  return t;
}

// What the 63-step verification kernel needs of a key (k_ate_key_prep, zkt_pairing.hip), kept for the last few keys like the tables above.  A key is served by that
// kernel only if its points lie in their groups AND its alpha_beta is the Tate pairing of its alpha and beta — the reference compares against the stored GTPoint
// (verifier.rs:48), so a key whose alpha_beta is anything else keeps the value-comparing kernels.  `usable` caches that verdict too.
//
// The entry is built at FIRST sight of a key, beside the call that brought it (round 4; before, at second sight and inside that call: 10 / 24 / 5 / 5 ms for the first four
// verifications against a key, now 10.5 / 5 / 5 / 5).  The pieces and where they run (timeline: profiles/r04_verify_first_sight_timeline.txt):
//   the two pairings of (alpha, beta), ONE launch of two blocks (k_key_ab, 4.8 ms)        -> the library's ONE guard stream (zkt_pairing.hip), from the start of the call: they need
//                                                                                            nothing but alpha and beta, and the guard stream is where pairing-sized frames may live
//   line tables of gamma and delta, group tests (k_ate_key_prep, 3 ms)                     -> a side stream for frames below 1 KB, from the start of the call
//   8-bit statement tables (k_stmt_wide_tables, 0.3 ms) from the points' 16^k tables        -> the same side stream, once the call's stream has built those (3 ms)
//   the verdict (flags, tate(alpha, beta)) into pinned host memory                          -> the guard stream, behind both; read by the next call on that key (ate_key_lookup)
// so a key's entry is complete ~5 ms into the call that first showed it, under that call's own 127-step kernels (which need nothing of the key); the call's guards queue behind
// the pairings on the guard stream (+0.5 ms on that one call).  A large batch, and zkt_groth16_vk_prepare, wait for the entry (5.5 ms instead of 21).
namespace {
struct AteHost { uint32_t flags; uint32_t pad[3]; uint64_t gt[72]; };
struct AteKey {
  std::vector<uint8_t> key, want_gt; std::shared_ptr<void> dev; bool usable = false; uint64_t stamp = 0;
  int state = 0;                       // 0 settled (or empty), 1 begun: side stream at work, pairings not enqueued, 2 pairings enqueued: verdict lands in *host when ev_done has passed
  hipEvent_t ev_in = nullptr, ev_side = nullptr, ev_done = nullptr; AteHost* host = nullptr; hipStream_t guard = nullptr;
};
std::mutex g_ate_mu; AteKey g_ate[4]; uint64_t g_ate_clock = 0; hipStream_t g_ate_side = nullptr;      // the side stream: kernels with frames below 1 KB only (scratch per queue, zkt_pairing.hip GuardStreams)
constexpr size_t ATE_TAIL_ALPHA = 0, ATE_TAIL_BETA = 28, ATE_TAIL_GT = 80, ATE_TAIL_WORDS = 224;      // behind the key words and the statement tables: alpha, beta, tate(alpha, beta)
std::vector<uint8_t> ate_key_bytes(const zkt_groth16_crs* c, size_t n_stmt) {
  std::vector<uint8_t> kb(G1B + 3 * G2B + 576 + n_stmt * G1B);
  uint8_t* w = kb.data();
  memcpy(w, c->g1_alpha, G1B); w += G1B; memcpy(w, c->g2_beta, G2B); w += G2B; memcpy(w, c->g2_gamma, G2B); w += G2B; memcpy(w, c->g2_delta, G2B); w += G2B;
  memcpy(w, c->gt_alpha_beta, 576); w += 576; memcpy(w, c->g1_uvw_stmt, n_stmt * G1B);
  return kb;
}
bool ate_key_applies(const zkt_groth16_crs* c, size_t n_stmt) {
  return n_stmt >= 1 && n_stmt <= 12 && c->g1_alpha && c->g2_beta;
}
void ate_settle_locked(AteKey& e) {                                   // state 2 -> 0: the verdict
  if (e.state != 2) return;
  const bool ok = hipEventSynchronize(e.ev_done) == hipSuccess;
  e.usable = ok && e.host->flags == 31u && memcmp(e.host->gt, e.want_gt.data(), 576) == 0;
  e.state = 0;
}
// First half (AteBuild::begin).  Returns the entry's index, or -1 (nothing started).  A begun entry MUST be followed by AteBuild::tables, or abandoned by its destructor.
int ate_key_begin(const zkt_groth16_crs* c, size_t n_stmt, const uint32_t* dU, const uint32_t* dg, const uint32_t* dd, hipStream_t s) {
  if (!ate_key_applies(c, n_stmt)) return -1;
  std::vector<uint8_t> kb = ate_key_bytes(c, n_stmt);
  std::lock_guard<std::mutex> lk(g_ate_mu);
  AteKey* victim = nullptr;
  for (AteKey& e : g_ate) {
    if (e.stamp && e.key == kb) return -1;                            // someone else got there first
    if (e.state == 0 && (!victim || e.stamp < victim->stamp)) victim = &e;
  }
  if (!victim) {                                                      // every entry still waits for its verdict (state 2 until a lookup of ITS key settles it): settle
    for (AteKey& e : g_ate) {                                         // them here, or four keys seen once each would hold the cache for the rest of the process
      ate_settle_locked(e);
      if (e.state == 0 && (!victim || e.stamp < victim->stamp)) victim = &e;
    }
  }
  if (!victim) return -1;
  AteKey& e = *victim;
  if (!g_ate_side && hipStreamCreateWithFlags(&g_ate_side, hipStreamNonBlocking) != hipSuccess) { g_ate_side = nullptr; (void)hipGetLastError(); return -1; }
  if (!e.ev_in && (hipEventCreateWithFlags(&e.ev_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e.ev_side, hipEventDisableTiming) != hipSuccess ||
                   hipEventCreateWithFlags(&e.ev_done, hipEventDisableTiming) != hipSuccess || hipHostMalloc((void**)&e.host, sizeof(AteHost)) != hipSuccess)) { (void)hipGetLastError(); return -1; }
  const size_t key_words = ATE_KEY_WORDS + stmt_wide_table_words((int)n_stmt);
  void* mem = nullptr;
  if (hipMalloc(&mem, (key_words + ATE_TAIL_WORDS) * 4) != hipSuccess) { (void)hipGetLastError(); return -1; }      // [line tables, alpha_beta, verdicts | statement tables | alpha, beta, tate(alpha, beta)]
  std::shared_ptr<void> dev(mem, [](void* q) { if (q) hipFree(q); });
  uint32_t* key = (uint32_t*)mem; uint32_t* tail = key + key_words;
  e.host->flags = 0; memset(e.host->gt, 0, 576);
  if (hipMemsetAsync(key + ATE_KEY_WORDS - 1, 0, 4, s) != hipSuccess || hipMemsetAsync(tail + ATE_TAIL_GT, 0, 576, s) != hipSuccess ||
      hipMemcpyAsync(tail + ATE_TAIL_ALPHA, c->g1_alpha, G1B, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(tail + ATE_TAIL_BETA, c->g2_beta, G2B, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipEventRecord(e.ev_in, s) != hipSuccess || hipStreamWaitEvent(g_ate_side, e.ev_in, 0) != hipSuccess ||
      launch_ate_key_prep(tail + ATE_TAIL_ALPHA, tail + ATE_TAIL_BETA, dg, dd, dU, (int)n_stmt, key, g_ate_side) != hipSuccess ||
      guard_fork(s, &e.guard) != hipSuccess ||
      launch_key_ab(tail + ATE_TAIL_ALPHA, tail + ATE_TAIL_BETA, key + ATE_KEY_TARGET, key + ATE_KEY_WORDS - 1, 16u, tail + ATE_TAIL_GT, e.guard) != hipSuccess) {
    (void)hipGetLastError(); (void)hipStreamSynchronize(g_ate_side); if (e.guard) (void)hipStreamSynchronize(e.guard); (void)hipStreamSynchronize(s); return -1;
  }
  e.key = std::move(kb); e.want_gt.assign((const uint8_t*)c->gt_alpha_beta, (const uint8_t*)c->gt_alpha_beta + 576); e.dev = dev; e.usable = false; e.stamp = ++g_ate_clock; e.state = 1;
  return (int)(victim - g_ate);
}
}  // namespace
void AteBuild::begin(const zkt_groth16_crs* c, size_t n_stmt, const uint32_t* dU, const uint32_t* dg, const uint32_t* dd, hipStream_t stream) { s = stream; idx = ate_key_begin(c, n_stmt, dU, dg, dd, s); }
// Second half, once `s` holds the statement points' 16^k tables: the 8-bit tables on the side stream, the verdict's way home on the guard stream behind both, and `s` waits for
// the side stream (whose kernels read the caller's per-call buffers, freed in stream order on `s`).
void AteBuild::tables(const uint32_t* tab16) {
  if (idx < 0) return;
  std::lock_guard<std::mutex> lk(g_ate_mu);
  AteKey& e = g_ate[idx]; idx = -1;
  uint32_t* key = (uint32_t*)e.dev.get(); const size_t n_stmt = (e.key.size() - (G1B + 3 * G2B + 576)) / G1B;
  uint32_t* tail = key + ATE_KEY_WORDS + stmt_wide_table_words((int)n_stmt);
  const bool ok = tab16 && hipEventRecord(e.ev_in, s) == hipSuccess && hipStreamWaitEvent(g_ate_side, e.ev_in, 0) == hipSuccess &&
                  launch_stmt_wide_tables(tab16, (int)n_stmt, key + ATE_KEY_WORDS, g_ate_side) == hipSuccess && hipEventRecord(e.ev_side, g_ate_side) == hipSuccess &&
                  hipStreamWaitEvent(e.guard, e.ev_side, 0) == hipSuccess && hipStreamWaitEvent(s, e.ev_side, 0) == hipSuccess &&
                  hipMemcpyAsync(&e.host->flags, key + ATE_KEY_WORDS - 1, 4, hipMemcpyDeviceToHost, e.guard) == hipSuccess &&
                  hipMemcpyAsync(e.host->gt, tail + ATE_TAIL_GT, 576, hipMemcpyDeviceToHost, e.guard) == hipSuccess && hipEventRecord(e.ev_done, e.guard) == hipSuccess;
  if (ok) { e.state = 2; return; }
  (void)hipGetLastError(); (void)hipStreamSynchronize(g_ate_side); (void)hipStreamSynchronize(e.guard); (void)hipStreamSynchronize(s);
  e.usable = false; e.state = 0;                                      // remembered as a key the 63-step loop does not serve
}
AteBuild::~AteBuild() {                                               // the call failed between begin and check: drain, forget
  if (idx < 0) return;
  std::lock_guard<std::mutex> lk(g_ate_mu);
  AteKey& e = g_ate[idx];
  (void)hipStreamSynchronize(g_ate_side); (void)hipStreamSynchronize(e.guard); (void)hipStreamSynchronize(s);
  e.dev.reset(); e.key.clear(); e.stamp = 0; e.usable = false; e.state = 0;
}
int ate_key_lookup(const zkt_groth16_crs* c, size_t n_stmt, std::shared_ptr<void>* out) {
  if (!ate_key_applies(c, n_stmt)) return ATE_UNUSABLE;
  const std::vector<uint8_t> kb = ate_key_bytes(c, n_stmt);
  std::lock_guard<std::mutex> lk(g_ate_mu);
  for (AteKey& e : g_ate) {
    if (!e.stamp || e.key != kb) continue;
    if (e.state == 1) return ATE_BUSY;
    ate_settle_locked(e);
    e.stamp = ++g_ate_clock;
    if (e.usable) { *out = e.dev; return ATE_READY; }
    return ATE_UNUSABLE;
  }
  return ATE_ABSENT;
}
std::shared_ptr<void> ate_key_now(const zkt_groth16_crs* c, size_t n_stmt, const uint32_t* dU, const uint32_t* dg, const uint32_t* dd, hipStream_t s) {
  std::shared_ptr<void> k;
  int st = ate_key_lookup(c, n_stmt, &k);
  if (st == ATE_ABSENT) {
    AteBuild b; b.begin(c, n_stmt, dU, dg, dd, s);
    if (b.idx < 0) return nullptr;
    const std::shared_ptr<void> tabs = stmt_tables_for(c->g1_uvw_stmt, n_stmt, dU, s);
    b.tables((const uint32_t*)tabs.get());
    st = ate_key_lookup(c, n_stmt, &k);                                // waits for the verdict; `tabs` is held until then
  }
  return st == ATE_READY ? k : nullptr;
}
}  // namespace zkt

using namespace zkt;
extern "C" void groth16_vk_clear_caches() {             // zkt_shutdown: device memory, events, pinned memory and the side stream held by the two caches
  { std::lock_guard<std::mutex> lk(g_stmt_mu); for (StmtTables& e : g_stmt) { e.tables.reset(); e.key.clear(); e.stamp = 0; } }
  { std::lock_guard<std::mutex> lk(g_ate_mu);
    for (AteKey& e : g_ate) {
      ate_settle_locked(e);
      if (e.ev_in) { (void)hipEventDestroy(e.ev_in); (void)hipEventDestroy(e.ev_side); (void)hipEventDestroy(e.ev_done); (void)hipHostFree(e.host); e.ev_in = e.ev_side = e.ev_done = nullptr; e.host = nullptr; }
      e.dev.reset(); e.key.clear(); e.stamp = 0; e.usable = false; e.state = 0;
    }
    if (g_ate_side) { (void)hipStreamSynchronize(g_ate_side); (void)hipStreamDestroy(g_ate_side); g_ate_side = nullptr; }
  }
}
