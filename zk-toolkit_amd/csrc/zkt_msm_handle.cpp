// The resident-base MSM handle of the C ABI (zkt_*_bases_*, zkt_*_msm_submit / _collect / _dev, zkt_*_msm_batch_*): a base set that stays on the
// device with its window-multiple table, eight pipeline slots and one batch in flight on streams of its own (or of the group it joined).
// Every device resource here is held by an owner whose destructor releases it; the rest of the library is reached through zkt_internal.h only.
#include <hip/hip_runtime.h>
#include <mutex>
#include <cstring>
#include <cstdlib>
#include "../../include/zkt.h"
#include "zkt_internal.h"
#include "host_abi.h"

using namespace zkt;

namespace {

// ---- owners of what Dev (host_abi.h) does not cover: each releases in its destructor and is never copied ------------------------------------
struct Pinned {                       // pinned host buffer
  uint8_t* p = nullptr;
  Pinned() = default;
  ~Pinned() { release(); }
  int alloc(size_t bytes) { HIPCHK(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault)); return ZKT_OK; }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; }
  Pinned(const Pinned&) = delete; Pinned& operator=(const Pinned&) = delete;
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  ~Event() { release(); }
  int create(bool timing) { if (!e) HIPCHK(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)); return ZKT_OK; }      // keeps the one it has
  void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  Event(const Event&) = delete; Event& operator=(const Event&) = delete;
};
struct Stream {                       // a stream the handle created, or one it borrowed from the owner of its group (left to that owner)
  hipStream_t s = nullptr;
  bool owned = false;
  Stream() = default;
  ~Stream() { if (owned && s) (void)hipStreamDestroy(s); }
  int create(int priority) { if (!s) { HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority)); owned = true; } return ZKT_OK; }   // keeps the one it has
  void borrow(const Stream& o) { s = o.s; owned = false; }
  Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
};

constexpr int MSM_SLOTS = 8;
// What one MSM pass in flight writes to, for `cap` scalar vectors: each of the eight slots has one with cap = 1, the batch has one that grows to the most
// vectors any batch had.  cap is set by reserve() after every member exists, and "ready for k vectors" is k <= cap: a half-built set has cap = 0.
struct InFlight {
  Dev workspace;                      // ws_bytes of the plan that runs on it
  Dev jac;                            // cap Jacobian partials, 3 coordinates each
  Dev abi;                            // cap ABI points
  Pinned host;                        // cap ABI points
  Event e_in, e_done;                 // inputs ready on the caller's stream / result complete (declared after the buffers: destroyed before them)
  int cap = 0, k = 0;                 // vectors the buffers hold / vectors of the pass in flight
  bool busy = false;
  void free_buffers() { workspace.release(); jac.release(); abi.release(); host.release(); cap = 0; }
  void clear() { free_buffers(); e_in.release(); e_done.release(); }
};
struct MsmSlot {                      // one in-flight MSM: its buffer set, the stage events of the three-stream pipeline, the graph cache of the one-stream pipeline
  InFlight set;
  Event e_sorted, e_acc0, e_acc1;
  // graph replay of a small MSM's pipeline (msm_submit): executable graphs captured on this slot, keyed by the scalar vector's address
  static constexpr int NGRAPH = 4;
  hipGraphExec_t gexec[NGRAPH] = {}; const void* gkey[NGRAPH] = {}; unsigned gnext = 0; bool timed = false;
};

}  // namespace

struct zkt_bases_impl {               // one resident base set of any group; zkt_g1_bases / zkt_g2_bases / zkt_secp_bases are this
  size_t n = 0;
  int grp = G_G1;
  MsmPlan plan{};
  Dev table;                          // nwin*n affine points, 2 internal coordinates each
  Dev inf;                            // nwin*n flags
  MsmSlot slot[MSM_SLOTS];
  InFlight batch;                     // the one in-flight batch (zkt_*_msm_batch_*): independent of the slots, created on the first batch
  // software pipeline: the three stages of consecutive MSMs run on three streams (sort | accumulate | reduce),
  // chained by events, so the atomic-bound sort and the latency-bound reduce of neighbours hide under the
  // VALU-bound accumulation of the current one.
  static constexpr int GROUP_TAILS = 4;   // reduce streams of a group of sets that share their streams (zkt_internal_bases_share_streams)
  static constexpr int NTAIL = 8;   // reduce chains of alternate MSMs run side by side: each is latency-bound, not throughput-bound (large MSMs use two of them)
  // a group of base sets that always work on the same job (the four sets of a Groth16 key) shares ONE set of streams: every stream beyond the
  // hardware queues (8) is folded onto a queue that already carries another stream, and a sort queued behind someone else's reduce chain waits for it
  // (measured: the A sum of a proof started 16 ms late behind the C1 reduce, profiles/r03_groth16_timeline.txt)
  Stream s_sort, s_acc, s_tail[NTAIL];   // declared after the slots and the batch: destroyed before their events and buffers
  bool grouped = false; int tail_base = 0, tail_span = 0;
  std::mutex mu;                 // slot state: calls on one handle are serialised (submit/collect of different slots may come from different threads)
  // Teardown, in the order it has to happen.  Freeing a handle with work in flight is legal use of the ABI.
  ~zkt_bases_impl() {
    // 1. wait for everything this handle queued: slots and batch in flight read the table and write the buffers below.  Every launch of the handle went to one of
    //    these streams, its own or borrowed (a borrower waits for the group's streams and leaves them to their owner, which is freed after it)
    for (Stream* st : {&s_sort, &s_acc}) if (st->s) (void)hipStreamSynchronize(st->s);
    for (Stream& st : s_tail) if (st.s) (void)hipStreamSynchronize(st.s);
    if (batch.busy) (void)hipEventSynchronize(batch.e_done.e);
    // 2. the executable graphs, which name the workspaces and were captured on the reduce streams: before either goes
    for (MsmSlot& S : slot) for (hipGraphExec_t& ge : S.gexec) if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
    // 3. events and owned streams, 4. buffers and the table: the members' destructors, in reverse order of declaration — the streams this handle owns
    //    (a borrower: at most its accumulate stream), then per buffer set its events and its buffers, then inf and table
  }
};
struct zkt_g1_bases : zkt_bases_impl {};
struct zkt_g2_bases : zkt_bases_impl {};
struct zkt_secp_bases : zkt_bases_impl {};

namespace {

// The streams of a handle, created where missing: sort and reduce high priority, accumulate low.  ntail reduce streams: NTAIL for a handle of its own,
// GROUP_TAILS for the owner of a group (exactly the streams the group uses: a stream that exists claims a hardware queue), 0 for a borrower that
// keeps an accumulate stream of its own beside the sort stream it borrowed.
int streams_create(zkt_bases_impl& h, int ntail) {
  int lo = 0, hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));        // hi = numerically smallest = highest priority
  ZCHK(h.s_sort.create(hi));
  ZCHK(h.s_acc.create(lo));
  for (int k = 0; k < ntail; ++k) ZCHK(h.s_tail[k].create(hi));
  return ZKT_OK;
}
int streams_ready(zkt_bases_impl& h) {      // on first use; a grouped handle got its streams from zkt_internal_bases_share_streams
  if (h.grouped || h.s_tail[zkt_bases_impl::NTAIL - 1].s) return ZKT_OK;      // the last one created
  return streams_create(h, zkt_bases_impl::NTAIL);
}
// The pipeline of an MSM below 2^19 terms is replayed as one graph launch per submit (msm_submit); ZKT_MSM_GRAPH=0 issues its launches one by one instead.
// Round 2 took this out because the 65,536-bit range-proof test aborted; round 3 found why (tools/diag/rp_graph.py): the captured graph held runtime-owned nodes — the
// hipMemsetAsync of the counters and the copy of the result — and replaying such a graph after ANY later hipFree in the process (a torch cache flush, a second context
// freeing its build scratch) ended in a memory access fault.  With kernel nodes only (k_zero_words clears the counters, the copy follows the graph on the stream) the
// replay survives all of that: every variant of the diagnostic, and the whole GPU suite, run in this mode.
bool msm_graphs() { static const bool on = [] { const char* e = getenv("ZKT_MSM_GRAPH"); return !(e && *e == '0'); }(); return on; }

hipStream_t slot_tail_stream(const zkt_bases_impl& h, int slot) {
  if (h.grouped) return h.s_tail[(h.tail_base + slot % h.tail_span) % zkt_bases_impl::GROUP_TAILS].s;      // a span may wrap around the group's four reduce streams
  const bool small = h.n < (size_t(1) << 19);
  return h.s_tail[small ? slot % zkt_bases_impl::NTAIL : slot % 2].s;
}
// the batch runs on the reduce stream of the last slot (a grouped handle: the group's stream for that slot)
hipStream_t batch_stream(const zkt_bases_impl& h) { return slot_tail_stream(h, MSM_SLOTS - 1); }

// Buffers of `F` for k vectors and a workspace of ws_bytes: nothing to do when it holds that many already (the submit path of a used slot), otherwise all of them
// or none — on any failure F is left empty.  st: the stream F's passes run on (a set that grows waits for it first).
int reserve(const zkt_bases_impl& h, InFlight& F, int k, size_t ws_bytes, hipStream_t st) {
  if (k <= F.cap) return ZKT_OK;
  if (F.cap) HIPCHK(hipStreamSynchronize(st));            // nothing of an earlier (collected) pass is still queued on the buffers about to go
  F.free_buffers();
  const auto build = [&]() -> int {
    ZCHK(F.e_in.create(false)); ZCHK(F.e_done.create(false));
    ZCHK(F.workspace.alloc(ws_bytes));
    if (debug_poison()) { HIPCHK(hipMemset(F.workspace.p, 0xA5, ws_bytes)); HIPCHK(hipDeviceSynchronize()); }
    ZCHK(F.jac.alloc((size_t)k * 3 * grp_coord_bytes(h.grp)));
    ZCHK(F.abi.alloc((size_t)k * abi_pt_bytes(h.grp)));
    return F.host.alloc((size_t)k * abi_pt_bytes(h.grp));
  };
  const int rc = build();
  if (rc) F.clear(); else F.cap = k;
  return rc;
}
// Result of the pass in flight on F: waits for it, then k ABI points to host `out` and k Jacobian partials to device `dev_partials` (either may be null)
int collect(const zkt_bases_impl& h, InFlight& F, hipStream_t st, void* out, uint32_t* dev_partials) {
  if (!F.busy) return ZKT_ERR_SHAPE;
  HIPCHK(hipEventSynchronize(F.e_done.e));
  if (dev_partials) {           // copied on the set's own stream and waited for: complete when this returns, and never overtaken by the next pass on the set
    HIPCHK(hipMemcpyAsync(dev_partials, F.jac.p, (size_t)F.k * 3 * grp_coord_bytes(h.grp), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (out) memcpy(out, F.host.p, (size_t)F.k * abi_pt_bytes(h.grp));
  F.busy = false;
  return ZKT_OK;
}
// the result copy and the completion event, behind the kernels of a pass on st
int finish_submit(const zkt_bases_impl& h, InFlight& F, int k, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(F.host.p, F.abi.p, (size_t)k * abi_pt_bytes(h.grp), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(F.e_done.e, st));
  F.k = k; F.busy = true;
  return ZKT_OK;
}

int slot_ready(zkt_bases_impl& h, int k) {   // lazily create the slot's events and workspace
  ZCHK(streams_ready(h));
  MsmSlot& S = h.slot[k];
  if (S.set.cap) return ZKT_OK;
  ZCHK(S.e_sorted.create(false)); ZCHK(S.e_acc0.create(true)); ZCHK(S.e_acc1.create(true));
  return reserve(h, S.set, 1, h.plan.ws_bytes, slot_tail_stream(h, k));
}

int bases_build(zkt_bases_impl& h, const uint32_t* dev_abi, hipStream_t s) {
  const size_t n = h.n, cb = grp_coord_bytes(h.grp);
  h.plan = msm_plan(n, h.grp);
  const size_t tot = (size_t)h.plan.nwin * (n ? n : 1);
  ZCHK(h.table.alloc(tot * 2 * cb));
  ZCHK(h.inf.alloc(tot));
  HIPCHK(launch_msm_to_kernel_layout(h.grp, dev_abi, h.table.w(), (uint8_t*)h.inf.p, n, s));
  Dev tmp;                                                   // Z and prefix products of the per-lane batched normalisation
  if (h.plan.nwin > 1) ZCHK(tmp.alloc((size_t)(h.plan.nwin - 1) * (n ? n : 1) * 2 * cb));
  hipError_t e = launch_msm_precompute(h.grp, h.table.w(), (uint8_t*)h.inf.p, n, h.plan.c, h.plan.nwin, tmp.w(), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);          // tmp is in use until here
  HIPCHK(e);
  return ZKT_OK;
}
int bases_from_device(int grp, const void* dev_bases, size_t n, void* stream, zkt_bases_impl** out) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!out || (n && !dev_bases) || n >= (size_t(1) << 26)) return ZKT_ERR_SHAPE;
  zkt_bases_impl* h = new zkt_bases_impl(); h->n = n; h->grp = grp;
  int rc = bases_build(*h, (const uint32_t*)dev_bases, (hipStream_t)stream);
  if (rc) { delete h; return rc; }
  *out = h; return ZKT_OK;
}
int bases_upload(int grp, const void* host, size_t n, zkt_bases_impl** out) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!out || (n && !host)) return ZKT_ERR_SHAPE;
  Dev tmp;
  ZCHK(tmp.alloc((n ? n : 1) * abi_pt_bytes(grp)));
  if (n) HIPCHK(hipMemcpy(tmp.p, host, n * abi_pt_bytes(grp), hipMemcpyHostToDevice));
  return bases_from_device(grp, tmp.p, n, zkt_internal_stream(), out);      // waits for the build before tmp goes
}

// ---- one MSM on a slot (caller holds h.mu) --------------------------------------------------------------------------------------------------
int msm_submit(zkt_bases_impl& h, const uint64_t* dev_scalars, size_t n, void* stream, int slot) {
  if (n != h.n || (n && !dev_scalars) || slot < 0 || slot >= MSM_SLOTS) return ZKT_ERR_SHAPE;
  if (h.slot[slot].set.busy) return ZKT_ERR_SHAPE;          // collect it first
  ZCHK(slot_ready(h, slot));
  MsmSlot& S = h.slot[slot];
  InFlight& F = S.set;
  // inputs are produced on the caller's stream: order the sort stage behind it
  HIPCHK(hipEventRecord(F.e_in.e, (hipStream_t)stream));
  const bool small = h.n < (size_t(1) << 19);       // (a set that shares a key's streams runs on the group's reduce stream for this slot: slot_tail_stream)
  hipStream_t st = slot_tail_stream(h, slot);
  hipStream_t ss = small ? st : h.s_sort.s;
  HIPCHK(hipStreamWaitEvent(ss, F.e_in.e, 0));
  if (small && msm_graphs()) {
    // A small MSM is ~20 launches of a few microseconds of GPU time each: the protocols that run several of them side by side (a range proof's five, a Pinocchio proof's
    // ten) are bound by the rate at which the host can submit them.  The whole pipeline of a slot — memsets, sort, accumulate, reduce, the copy of the result — touches only
    // the slot's own buffers and the scalar vector (kernel launches only: the counters are cleared by a kernel of the pipeline's own), so it is captured ONCE per (slot, scalar address) on the slot's stream and replayed as one graph launch.  Nothing inside
    // the capture waits on or records an event (the input dependency is the stream wait above, completion is e_done below); the slot is not busy here, so no launch of an
    // executable graph that gets evicted is still in flight.
    int hit = -1;
    for (int k = 0; k < MsmSlot::NGRAPH; ++k) if (S.gexec[k] && S.gkey[k] == (const void*)dev_scalars) hit = k;
    if (hit < 0) {
      hit = (int)(S.gnext++ % MsmSlot::NGRAPH);
      if (S.gexec[hit]) { (void)hipGraphExecDestroy(S.gexec[hit]); S.gexec[hit] = nullptr; }
      hipGraph_t graph = nullptr;
      HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
      hipError_t e = launch_msm_sort(h.plan, (const uint8_t*)h.inf.p, (const uint32_t*)dev_scalars, F.workspace.p, st);
      if (e == hipSuccess) e = launch_msm_accumulate(h.plan, h.table.w(), F.workspace.p, st);
      if (e == hipSuccess) e = launch_msm_reduce(h.plan, F.workspace.p, F.jac.w(), F.abi.w(), st);
      const hipError_t e2 = hipStreamEndCapture(st, &graph);                 // always: the stream must leave capture mode
      if (e != hipSuccess || e2 != hipSuccess || !graph) { if (graph) (void)hipGraphDestroy(graph); HIPCHK(e != hipSuccess ? e : (e2 != hipSuccess ? e2 : hipErrorUnknown)); }
      e = hipGraphInstantiate(&S.gexec[hit], graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (e != hipSuccess) { S.gexec[hit] = nullptr; HIPCHK(e); }
      S.gkey[hit] = (const void*)dev_scalars;
    }
    HIPCHK(hipGraphLaunch(S.gexec[hit], st));
    S.timed = false;
    return finish_submit(h, F, 1, st);      // kernels only inside the graph: the copy of the result follows it on the stream
  }
  S.timed = true;
  HIPCHK(launch_msm_sort(h.plan, (const uint8_t*)h.inf.p, (const uint32_t*)dev_scalars, F.workspace.p, ss));
  HIPCHK(hipEventRecord(S.e_sorted.e, ss));
  // a large MSM fills the chip, so its stages queue on per-stage streams (sort of MSM k+1 under the accumulation of MSM k); below 2^19 terms every
  // stage is a latency-bound sliver of the chip (one short wave per SIMD), so each slot runs its whole MSM on its own stream, side by side with the others
  hipStream_t sa = small ? st : h.s_acc.s;
  HIPCHK(hipStreamWaitEvent(sa, S.e_sorted.e, 0));
  HIPCHK(hipEventRecord(S.e_acc0.e, sa));
  HIPCHK(launch_msm_accumulate(h.plan, h.table.w(), F.workspace.p, sa));
  HIPCHK(hipEventRecord(S.e_acc1.e, sa));
  HIPCHK(hipStreamWaitEvent(st, S.e_acc1.e, 0));
  HIPCHK(launch_msm_reduce(h.plan, F.workspace.p, F.jac.w(), F.abi.w(), st));
  return finish_submit(h, F, 1, st);
}
int msm_collect(zkt_bases_impl& h, int slot, void* out, uint32_t* dev_partial_jac) {
  if (slot < 0 || slot >= MSM_SLOTS) return ZKT_ERR_SHAPE;
  MsmSlot& S = h.slot[slot];
  ZCHK(collect(h, S.set, slot_tail_stream(h, slot), out, dev_partial_jac));
  float ms = 0.f;
  if (S.timed && hipEventElapsedTime(&ms, S.e_acc0.e, S.e_acc1.e) == hipSuccess) zkt_internal_set_last_kernel(ms, "k_accumulate");
  else zkt_internal_set_last_kernel(0.f, "msm_graph");      // a graph-replayed MSM carries no per-kernel events: say so instead of leaving the previous operation's figures
  return ZKT_OK;
}
// ---- batched form: k scalar vectors over the handle's base set in ONE pipeline (msm_plan_batch; caller holds h.mu) ---------------------------------
// Below 2^19 terms every kernel of an MSM is a latency-bound sliver of the chip, and k MSMs on k slots are k chains of ~20 such kernels side by side.  The batch
// runs ONE chain whose grids cover all k vectors: bucket set v for vector v, one task list, one accumulate launch, the reduce kernels with grid.y = k.
// It has a buffer set and a completion event of its own, so slot MSMs and a batch may be in flight on one handle together; it runs on the reduce
// stream of the last slot (batch_stream), issued launch by launch — no graph (profiles/msm_batch_go_no_go.md).
int msm_batch_submit(zkt_bases_impl& h, const uint64_t* dev_scalars, size_t n, size_t k, size_t vec_stride, void* stream) {
  if (n != h.n || k == 0 || k > ZKT_MSM_BATCH_MAX || vec_stride < n || n >= (size_t(1) << 19) || k * n > ZKT_MSM_BATCH_MAX_TERMS || (n && !dev_scalars)) return ZKT_ERR_SHAPE;
  InFlight& F = h.batch;
  if (F.busy) return ZKT_ERR_SHAPE;               // collect it first
  const MsmPlan P = msm_plan_batch(n, h.grp, (int)k);
  if (P.c != h.plan.c || P.nwin != h.plan.nwin || P.nbuckets > (size_t(1) << 21)) return ZKT_ERR_SHAPE;      // the entries index the table the handle was built with
  ZCHK(streams_ready(h));
  hipStream_t st = batch_stream(h);
  ZCHK(reserve(h, F, (int)k, P.ws_bytes, st));     // allocates on the first batch and when k exceeds every earlier one
  HIPCHK(hipEventRecord(F.e_in.e, (hipStream_t)stream));   // the scalars are produced on the caller's stream
  HIPCHK(hipStreamWaitEvent(st, F.e_in.e, 0));
  HIPCHK(launch_msm_sort_batch(P, (const uint8_t*)h.inf.p, (const uint32_t*)dev_scalars, vec_stride, F.workspace.p, st));
  HIPCHK(launch_msm_accumulate(P, h.table.w(), F.workspace.p, st));
  HIPCHK(launch_msm_reduce(P, F.workspace.p, F.jac.w(), F.abi.w(), st));
  return finish_submit(h, F, (int)k, st);
}
int msm_batch_collect(zkt_bases_impl& h, void* out, uint32_t* dev_partials_jac) {
  ZCHK(collect(h, h.batch, batch_stream(h), out, dev_partials_jac));
  zkt_internal_set_last_kernel(0.f, "msm_batch");
  return ZKT_OK;
}

// every entry point that works on a handle: the library is ready, the handle (and whatever else `args_ok` says) is there, the handle's lock is held.
// The blocking forms submit and collect under one hold of it (two threads may share a handle).
template <class Fn> int with_handle(const zkt_bases_impl* b, bool args_ok, Fn f) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!b || !args_ok) return ZKT_ERR_SHAPE;
  zkt_bases_impl& h = *const_cast<zkt_bases_impl*>(b);
  std::lock_guard<std::mutex> lk(h.mu);
  return f(h);
}

}  // namespace

extern "C" {

// `dst` works on `src`'s streams from now on (sort stream and reduce streams [tail_base, tail_base + tail_span); the accumulate stream too if share_acc,
// otherwise dst gets one of its own).  Call before dst's first MSM; free dst before src.
int zkt_internal_bases_share_streams(void* dst_, void* src_, int share_acc, int tail_base, int tail_span) {
  zkt_bases_impl *dst = (zkt_bases_impl*)dst_, *src = (zkt_bases_impl*)src_;
  if (!dst || !src || tail_span < 1 || tail_base < 0) return ZKT_ERR_SHAPE;
  constexpr int GROUP_TAILS = zkt_bases_impl::GROUP_TAILS;
  if (tail_base >= GROUP_TAILS || tail_span > GROUP_TAILS) return ZKT_ERR_SHAPE;
  {
    std::lock_guard<std::mutex> lk(src->mu);
    if (!src->grouped) {                       // the owner
      if (src->s_sort.s || src->s_acc.s) return ZKT_ERR_SHAPE;
      ZCHK(streams_create(*src, GROUP_TAILS));
      src->grouped = true; src->tail_base = 0; src->tail_span = 2;
    }
  }
  std::lock_guard<std::mutex> lk(dst->mu);
  if (dst->s_sort.s || dst->s_acc.s) return ZKT_ERR_SHAPE;
  dst->grouped = true; dst->s_sort.borrow(src->s_sort);
  for (int k = 0; k < GROUP_TAILS; ++k) dst->s_tail[k].borrow(src->s_tail[k]);
  dst->tail_base = tail_base; dst->tail_span = tail_span;
  if (share_acc) dst->s_acc.borrow(src->s_acc);
  else ZCHK(streams_create(*dst, 0));          // the accumulate stream is the one it lacks
  return ZKT_OK;
}

#define ZKT_BASES_API(NAME, GRP, PT)                                                                                             \
  int zkt_##NAME##_bases_from_device(const PT* dev, size_t n, void* stream, zkt_##NAME##_bases** out) {                          \
    return bases_from_device(GRP, dev, n, stream, (zkt_bases_impl**)out); }                                                     \
  int zkt_##NAME##_bases_upload(const PT* host, size_t n, zkt_##NAME##_bases** out) { return bases_upload(GRP, host, n, (zkt_bases_impl**)out); } \
  size_t zkt_##NAME##_bases_len(const zkt_##NAME##_bases* b) { return b ? b->n : 0; }                                             \
  void zkt_##NAME##_bases_free(zkt_##NAME##_bases* b) { delete static_cast<zkt_bases_impl*>(b); }                                                              \
  int zkt_##NAME##_msm_submit(zkt_##NAME##_bases* b, const uint64_t* k, size_t n, void* stream, int slot) {                      \
    return with_handle(b, true, [&](zkt_bases_impl& h) { return msm_submit(h, k, n, stream, slot); }); }                        \
  int zkt_##NAME##_msm_collect(zkt_##NAME##_bases* b, int slot, PT* out, uint32_t* partial) {                                    \
    return with_handle(b, true, [&](zkt_bases_impl& h) { return msm_collect(h, slot, out, partial); }); }                       \
  int zkt_##NAME##_msm_dev(const zkt_##NAME##_bases* b, const uint64_t* k, size_t n, void* stream, PT* out, uint32_t* partial) { \
    return with_handle(b, out || partial, [&](zkt_bases_impl& h) {                              /* slot 0 */                   \
      ZCHK(msm_submit(h, k, n, stream, 0)); return msm_collect(h, 0, out, partial); }); }                                       \
  int zkt_##NAME##_msm_batch_submit(zkt_##NAME##_bases* b, const uint64_t* k, size_t n, size_t nv, size_t vs, void* stream) {    \
    return with_handle(b, true, [&](zkt_bases_impl& h) { return msm_batch_submit(h, k, n, nv, vs, stream); }); }                \
  int zkt_##NAME##_msm_batch_collect(zkt_##NAME##_bases* b, PT* out, uint32_t* partials) {                                       \
    return with_handle(b, true, [&](zkt_bases_impl& h) { return msm_batch_collect(h, out, partials); }); }                      \
  int zkt_##NAME##_msm_batch_dev(zkt_##NAME##_bases* b, const uint64_t* k, size_t n, size_t nv, size_t vs, void* stream, PT* out, uint32_t* partials) { \
    return with_handle(b, out || partials, [&](zkt_bases_impl& h) {                                                             \
      ZCHK(msm_batch_submit(h, k, n, nv, vs, stream)); return msm_batch_collect(h, out, partials); }); }
ZKT_BASES_API(g1, G_G1, zkt_g1_affine)
ZKT_BASES_API(g2, G_G2, zkt_g2_affine)
ZKT_BASES_API(secp, G_SECP, zkt_secp_affine)
size_t zkt_g1_msm_workspace_bytes(size_t n) { MsmPlan p = msm_plan(n, G_G1); return p.ws_bytes + (size_t)p.nwin * n * 97; }

}  // extern "C"
