// C ABI (include/zkt.h) over the HIP kernels: init and shutdown, fields, towers, groups, pairings and the one-shot MSM.  Host-pointer entry points stage
// through a grow-only device arena, one Stage (host_stage.h) per call; `_dev` entry points launch on the caller's stream.  There is
// no CPU compute path in this file: without a device every entry point fails.
// The resident-base MSM handle (zkt_*_bases_*, zkt_*_msm_submit / _collect / _dev, zkt_*_msm_batch_*) is zkt_msm_handle.cpp; the hash and signature
// entry points (zkt_sha256 / sha512 / ecdsa / ed25519_*) are zkt_hashsig.cpp.
#include <hip/hip_runtime.h>
#include <mutex>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include "../../include/zkt.h"
#include "zkt_internal.h"
#include "zkt_constants.h"
#include "host_abi.h"
#include "host_stage.h"
static_assert(ZKT_G1_PARTIAL_WORDS == 3 * zkt::FqC::N && ZKT_G2_PARTIAL_WORDS == 6 * zkt::FqC::N && ZKT_SECP_PARTIAL_WORDS == 3 * zkt::SpC::N,
              "include/zkt.h partial sizes follow the internal limb layout");

using namespace zkt;

namespace {

struct Ctx {
  bool ready = false;
  int device = -1;
  hipStream_t stream = nullptr;
  unsigned long long* d_err = nullptr;
  uint8_t* arena = nullptr; size_t arena_bytes = 0;
  uint32_t* d_small = nullptr;          // 4 KB of device scratch for one-point results (caller holds mu)
  std::mutex mu;
};
Ctx g;
thread_local size_t t_err_index = 0;
thread_local float t_kernel_ms = 0.f;
thread_local const char* t_kernel_name = "";

// every entry point starts here: the library owns ONE device (zkt_init), and a thread's current HIP device is per-thread state,
// so it is set on entry — handles, streams and workspaces are then always created and used on that device
int ensure_ready() {
  if (!g.ready) return ZKT_ERR_DEVICE;
  return hipSetDevice(g.device) == hipSuccess ? ZKT_OK : ZKT_ERR_DEVICE;
}

// grow-only staging arena (caller holds g.mu: Stage::commit)
int arena_reserve(size_t bytes) {
  if (bytes <= g.arena_bytes) return ZKT_OK;
  if (g.arena) { HIPCHK(hipFree(g.arena)); g.arena = nullptr; g.arena_bytes = 0; }
  size_t want = bytes + (bytes >> 2) + (1 << 20);
  HIPCHK(hipMalloc((void**)&g.arena, want));
  g.arena_bytes = want;
  return ZKT_OK;
}
size_t padded(size_t b) { return (b + 255) & ~size_t(255); }      // the blob of msm_host
// the point at infinity in the ABI layout of a w-byte point: all zero, flag word 1
void set_infinity(void* out, size_t w) { memset(out, 0, w); ((uint32_t*)out)[w / 4 - 2] = 1; }

int reset_err(hipStream_t s) {
  unsigned long long v = NO_ERR;
  HIPCHK(hipMemcpyAsync(g.d_err, &v, sizeof(v), hipMemcpyHostToDevice, s));
  return ZKT_OK;
}
int fetch_err(hipStream_t s, int code_if_set) {
  unsigned long long v = NO_ERR;
  HIPCHK(hipMemcpyAsync(&v, g.d_err, sizeof(v), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (v != NO_ERR) { t_err_index = (size_t)v; return code_if_set; }
  return ZKT_OK;
}

// generic host-staged op: in_a, in_b (optional) -> out, sizes in bytes
template <class Launch>
int staged_raw(const void* a, size_t a_total, const void* b, size_t b_total, void* out, size_t out_total, int err_code, Launch launch) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!a || !out || (b_total && !b)) return ZKT_ERR_SHAPE;
  Stage st;
  const int ia = st.in(a, a_total), ib = b_total ? st.in(b, b_total) : Stage::NONE, io = st.out(out, out_total);
  ZCHK(st.commit());
  ZCHK(reset_err(g.stream));
  HIPCHK(launch(st.ptr<uint32_t>(ia), st.ptr<uint32_t>(ib), st.ptr<uint32_t>(io), g.stream));
  return st.finish_err(err_code);
}
// elementwise form: fixed bytes per element
template <class Launch>
int staged(const void* a, size_t a_bytes, const void* b, size_t b_bytes, void* out, size_t out_bytes, size_t n, int err_code, Launch launch) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (n == 0) return ZKT_OK;
  return staged_raw(a, a_bytes * n, b, b_bytes * n, out, out_bytes * n, err_code, launch);
}

size_t field_bytes(int field) { return field == F_FQ ? 48 : 32; }
int fp_batch(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const size_t w = field_bytes(field);
  const bool binary = op == OP_ADD || op == OP_SUB || op == OP_MUL;
  return staged(a, w, binary ? b : nullptr, binary ? w : 0, out, w, n, ZKT_ERR_INV_ZERO,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_fp_op(field, op, da, db, dout, n, g.d_err, s); });
}
// a3: pow with per-element or shared exponents of exp_limbs u64 limbs; pow_seq / repeat from one base element
int fp_pow_batch(int field, const uint64_t* a, const uint64_t* exps, size_t exp_limbs, int exp_shared, uint64_t* out, size_t n) {
  if (exp_limbs == 0 || exp_limbs > 64) return ZKT_ERR_SHAPE;
  if (n == 0) return ensure_ready();
  const size_t w = field_bytes(field);
  return staged_raw(a, w * n, exps, exp_limbs * 8 * (exp_shared ? 1 : n), out, w * n, ZKT_ERR_SHAPE,
                    [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_fp_pow(field, da, db, (int)exp_limbs * 2, exp_shared != 0, dout, n, s); });
}
int fp_pow_seq(int field, const uint64_t* base, size_t n, uint64_t* out, bool repeat) {
  if (n == 0) return ensure_ready();
  const size_t w = field_bytes(field);
  return staged_raw(base, w, nullptr, 0, out, w * n, ZKT_ERR_SHAPE,
                    [&](uint32_t* da, uint32_t*, uint32_t* dout, hipStream_t s) { return launch_fp_pow_seq(field, da, dout, n, repeat, s); });
}
// a18's vector forms: PrimeFieldElems::sum (prime_field_elems.rs:35-41, panics on an empty vector) and PrimeFieldElems * PrimeFieldElem (:152-175)
int fp_sum(int field, const uint64_t* a, size_t n, uint64_t* out) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (n == 0 || !a || !out) return ZKT_ERR_SHAPE;                    // assert!(self.0.len() > 0)
  const size_t w = field_bytes(field);
  Stage st;
  const int ia = st.in(a, w * n), io = st.out(out, w), ip = st.scratch(w * fp_sum_scratch_elems());
  ZCHK(st.commit());
  HIPCHK(launch_fp_sum(field, st.ptr<uint32_t>(ia), n, st.ptr<uint32_t>(io), st.ptr<uint32_t>(ip), g.stream));
  return st.finish();
}
int fp_scale(int field, const uint64_t* a, const uint64_t* k, uint64_t* out, size_t n) {
  if (n == 0) return ZKT_ERR_SHAPE;                                  // assert!(self.len() > 0)
  const size_t w = field_bytes(field);
  return staged_raw(a, w * n, k, w, out, w * n, ZKT_ERR_SHAPE,
                    [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_fp_scale(field, da, db, dout, n, s); });
}
int tower_batch(int deg, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const size_t w = (size_t)deg * 48;
  const bool binary = op == T_ADD || op == T_SUB || op == T_MUL;
  return staged(a, w, binary ? b : nullptr, binary ? w : 0, out, w, n, ZKT_ERR_INV_ZERO,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_tower_op(deg, op, da, db, dout, n, g.d_err, s); });
}

}  // namespace

// ---- Stage (host_stage.h): the parts that touch the arena, the lock and the error word ----
Stage::Stage() : lock_(g.mu), stream_(g.stream), small_(g.d_small) {}
int Stage::commit() {
  ZCHK(arena_reserve(stage_layout(bytes_, n_, off_)));
  base_ = g.arena;
  for (int i = 0; i < n_; ++i)
    if (src_[i] && bytes_[i]) HIPCHK(hipMemcpyAsync(base_ + off_[i], src_[i], bytes_[i], hipMemcpyHostToDevice, stream_));
  return ZKT_OK;
}
int Stage::downloads() {
  for (int i = 0; i < n_; ++i)
    if (dst_[i] && dst_bytes_[i]) HIPCHK(hipMemcpyAsync(dst_[i], base_ + off_[i], dst_bytes_[i], hipMemcpyDeviceToHost, stream_));
  return ZKT_OK;
}
int Stage::finish() {
  ZCHK(downloads());
  HIPCHK(hipStreamSynchronize(stream_));
  return ZKT_OK;
}
int Stage::finish_err(int code_if_set) {
  ZCHK(downloads());
  return fetch_err(stream_, code_if_set);
}

int zkt_internal_ready() { return ensure_ready(); }
hipStream_t zkt_internal_stream() { return g.stream; }
int zkt_internal_device() { return g.device; }
void zkt_internal_set_error_index(size_t i) { t_err_index = i; }
void zkt_internal_set_last_kernel(float ms, const char* name) { t_kernel_ms = ms; t_kernel_name = name; }

extern "C" {

int zkt_version(void) { return 1; }
const char* zkt_strerror(int s) {
  switch (s) {
    case ZKT_OK: return "ok";
    case ZKT_ERR_INV_ZERO: return "Cannot find inverse of zero";
    case ZKT_ERR_INFINITY: return "pairing argument is the point at infinity";
    case ZKT_ERR_SHAPE: return "bad size, null pointer or non-canonical input";
    case ZKT_ERR_DEVICE: return "no HIP device / HIP error / zkt_init not called";
    case ZKT_ERR_REMAINDER: return "p should be divisible by t";
  }
  return "unknown";
}
size_t zkt_last_error_index(void) { return t_err_index; }
float zkt_last_kernel_ms(void) { return t_kernel_ms; }
const char* zkt_last_kernel_name(void) { return t_kernel_name; }

int zkt_init(int device) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (g.ready) return ZKT_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { fprintf(stderr, "[zkt] no HIP device: this library has no CPU path\n"); return ZKT_ERR_DEVICE; }
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return ZKT_ERR_DEVICE; }
  if (device >= count) return ZKT_ERR_DEVICE;
  HIPCHK(hipSetDevice(device));
  g.device = device;
  HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  HIPCHK(hipMalloc((void**)&g.d_err, 64));
  HIPCHK(hipMalloc((void**)&g.d_small, 4096));
  g.ready = true;
  return ZKT_OK;
}
static void tate_events_release();
void zkt_shutdown(void) {
  if (g.ready) (void)hipSetDevice(g.device);
  zkt_comm_finalize();                                // the communicator and its buffers live on this device
  zkt_poly_clear_caches();                            // twiddle tables of the polynomial entry points
  zkt_pinocchio_clear_caches(); bp_clear_caches(); groth16_vk_clear_caches();      // before g.mu is taken: releasing a cached context frees base sets, which lock it themselves
  std::lock_guard<std::mutex> lk(g.mu);
  if (!g.ready) return;
  (void)hipSetDevice(g.device);
  group_release_device_state();                       // generator comb tables
  ed25519_release_device_state();                     // the comb table of the Ed25519 base point
  pairing_release_device_state();                     // guard side stream + events
  tate_events_release();
  if (g.arena) (void)hipFree(g.arena);
  if (g.d_err) (void)hipFree(g.d_err);
  if (g.d_small) (void)hipFree(g.d_small);
  if (g.stream) (void)hipStreamDestroy(g.stream);
  g.ready = false; g.device = -1; g.stream = nullptr; g.d_err = nullptr; g.d_small = nullptr; g.arena = nullptr; g.arena_bytes = 0;
}

#define FP_BIN(name, field, op) int name(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) { return fp_batch(field, op, a, b, out, n); }
#define FP_UN(name, field, op) int name(const uint64_t* a, uint64_t* out, size_t n) { return fp_batch(field, op, a, nullptr, out, n); }
// the four prime fields the reference instantiates: BLS12-381 Fq and Fr, secp256k1's base field (sp) and group order (sn)
#define FP_FIELD_API(P, F)                                                                                       \
  FP_BIN(zkt_##P##_add_batch, F, OP_ADD) FP_BIN(zkt_##P##_sub_batch, F, OP_SUB) FP_BIN(zkt_##P##_mul_batch, F, OP_MUL) \
  FP_UN(zkt_##P##_sqr_batch, F, OP_SQR) FP_UN(zkt_##P##_neg_batch, F, OP_NEG) FP_UN(zkt_##P##_inv_batch, F, OP_INV)     \
  FP_UN(zkt_##P##_cube_batch, F, OP_CUBE)                                                                        \
  int zkt_##P##_pow_batch(const uint64_t* a, const uint64_t* exps, size_t exp_limbs, int exp_shared, uint64_t* out, size_t n) { \
    return fp_pow_batch(F, a, exps, exp_limbs, exp_shared, out, n); }                                            \
  int zkt_##P##_sum(const uint64_t* a, size_t n, uint64_t* out) { return fp_sum(F, a, n, out); }                   \
  int zkt_##P##_scale_batch(const uint64_t* a, const uint64_t* k, uint64_t* out, size_t n) { return fp_scale(F, a, k, out, n); } \
  int zkt_##P##_pow_seq(const uint64_t* base, size_t n, uint64_t* out) { return fp_pow_seq(F, base, n, out, false); }  \
  int zkt_##P##_repeat(const uint64_t* base, size_t n, uint64_t* out) { return fp_pow_seq(F, base, n, out, true); }
FP_FIELD_API(fq, F_FQ) FP_FIELD_API(fr, F_FR) FP_FIELD_API(sp, F_SP) FP_FIELD_API(sn, F_SN)

#define TW_BIN(name, deg, op) int name(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) { return tower_batch(deg, op, a, b, out, n); }
#define TW_UN(name, deg, op) int name(const uint64_t* a, uint64_t* out, size_t n) { return tower_batch(deg, op, a, nullptr, out, n); }
TW_BIN(zkt_fq2_add_batch, 2, T_ADD) TW_BIN(zkt_fq2_sub_batch, 2, T_SUB) TW_BIN(zkt_fq2_mul_batch, 2, T_MUL)
TW_UN(zkt_fq2_inv_batch, 2, T_INV) TW_UN(zkt_fq2_neg_batch, 2, T_NEG) TW_UN(zkt_fq2_reduce_batch, 2, T_REDUCE)
TW_BIN(zkt_fq6_add_batch, 6, T_ADD) TW_BIN(zkt_fq6_sub_batch, 6, T_SUB) TW_BIN(zkt_fq6_mul_batch, 6, T_MUL)
TW_UN(zkt_fq6_inv_batch, 6, T_INV) TW_UN(zkt_fq6_neg_batch, 6, T_NEG) TW_UN(zkt_fq6_reduce_batch, 6, T_REDUCE)
TW_BIN(zkt_fq12_add_batch, 12, T_ADD) TW_BIN(zkt_fq12_sub_batch, 12, T_SUB) TW_BIN(zkt_fq12_mul_batch, 12, T_MUL)
TW_UN(zkt_fq12_inv_batch, 12, T_INV) TW_UN(zkt_fq12_neg_batch, 12, T_NEG)

int zkt_fq12_pow_batch(const uint64_t* a, const uint32_t* e, size_t nl, uint64_t* out, size_t n) {
  if (!e || nl == 0 || nl > 4096) return ZKT_ERR_SHAPE;
  // the exponent rides in front of the `a` staging area as a second input of fixed size
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (n == 0) return ZKT_OK;
  if (!a || !out) return ZKT_ERR_SHAPE;
  Stage st;
  const int ia = st.in(a, 576 * n), io = st.out(out, 576 * n), ie = st.in(e, nl * 4);
  ZCHK(st.commit());
  HIPCHK(launch_fq12_pow(st.ptr<uint32_t>(ia), st.ptr<uint32_t>(ie), (int)nl, st.ptr<uint32_t>(io), n, g.stream));
  return st.finish();
}

// diagnostic: the lazy-limb Fq self-test program (fq_program.h) on the device, one run per lane
int zkt_selftest_fq_program(uint64_t seed0, int steps, const uint64_t* in, uint64_t* out, int32_t* violations, size_t count) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (count == 0) return ZKT_OK;
  if (!in || !out || !violations || steps < 0) return ZKT_ERR_SHAPE;
  const size_t eb = 4 * 48;
  Stage st;
  const int ii = st.in(in, eb * count), io = st.out(out, eb * count), ib = st.out(violations, 4 * count);
  ZCHK(st.commit());
  HIPCHK(launch_selftest_fq_program(seed0, steps, st.ptr<uint32_t>(ii), st.ptr<uint32_t>(io), st.ptr<int>(ib), count, g.stream));
  return st.finish();
}

// diagnostic: Fq12 operations of the lane-distributed pairing (zkt_dpairing.hip), same layouts as zkt_fq12_*_batch
int zkt_debug_dfq12_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (op < 0 || op > 6) return ZKT_ERR_SHAPE;
  return staged(a, 576, op == 0 ? b : nullptr, op == 0 ? 576 : 0, out, 576, n, ZKT_ERR_SHAPE,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_dfq12_op(op, da, db, dout, n, s); });
}

static int group_add(int grp, const void* a, const void* b, void* out, size_t n) {
  size_t w = abi_pt_bytes(grp);
  return staged(a, w, b, w, out, w, n, ZKT_ERR_SHAPE,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_group_add(grp, da, db, dout, n, s); });
}
static int group_neg(int grp, const void* a, void* out, size_t n) {
  size_t w = abi_pt_bytes(grp);
  return staged(a, w, nullptr, 0, out, w, n, ZKT_ERR_SHAPE,
                [&](uint32_t* da, uint32_t*, uint32_t* dout, hipStream_t s) { return launch_group_neg(grp, da, dout, n, s); });
}
static int group_mul(int grp, const void* pts, const uint64_t* scalars, int limbs, void* out, size_t n) {
  if (limbs < 1 || limbs > 6) return ZKT_ERR_SHAPE;
  size_t w = abi_pt_bytes(grp);
  return staged(pts, w, scalars, (size_t)limbs * 8, out, w, n, ZKT_ERR_SHAPE,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_group_mul(grp, da, db, limbs * 2, dout, n, s); });
}
// AffinePoints::sum (secp256k1/affine_points.rs:25-31: the fold from AffinePoint::zero(), so an empty vector sums to infinity) and
// AffinePoints * PrimeFieldElem (:105-122): every point times ONE scalar
static int group_sum(int grp, const void* pts, size_t n, void* out) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  const size_t w = abi_pt_bytes(grp);
  if (!out || (n && !pts)) return ZKT_ERR_SHAPE;
  if (n == 0) { set_infinity(out, w); return ZKT_OK; }
  alignas(8) uint8_t pair[2 * G2B];                                  // lives until the call's last wait
  if (n == 1) {                                                      // p + zero: goes through the addition so that the coordinates come back reduced
    memcpy(pair, pts, w); set_infinity(pair + w, w);
    pts = pair; n = 2;
  }
  Stage st;
  const int ia = st.inout(pts, w * n, out, w);
  ZCHK(st.commit());
  HIPCHK(launch_group_sum_inplace(grp, st.ptr<uint32_t>(ia), n, g.stream));       // result in the first point
  return st.finish();
}
static int group_scale(int grp, const void* pts, const uint64_t* k, int limbs, void* out, size_t n) {
  if (limbs < 1 || limbs > 6) return ZKT_ERR_SHAPE;
  if (n == 0) return ensure_ready();
  size_t w = abi_pt_bytes(grp);
  return staged_raw(pts, w * n, k, (size_t)limbs * 8, out, w * n, ZKT_ERR_SHAPE,
                    [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_group_mul(grp, da, db, limbs * 2, dout, n, s, false, true); });
}
int zkt_g1_sum(const zkt_g1_affine* p, size_t n, zkt_g1_affine* o) { return group_sum(G_G1, p, n, o); }
int zkt_g2_sum(const zkt_g2_affine* p, size_t n, zkt_g2_affine* o) { return group_sum(G_G2, p, n, o); }
int zkt_secp_sum(const zkt_secp_affine* p, size_t n, zkt_secp_affine* o) { return group_sum(G_SECP, p, n, o); }
int zkt_g1_scale_batch(const zkt_g1_affine* p, const uint64_t* k, int l, zkt_g1_affine* o, size_t n) { return group_scale(G_G1, p, k, l, o, n); }
int zkt_g2_scale_batch(const zkt_g2_affine* p, const uint64_t* k, int l, zkt_g2_affine* o, size_t n) { return group_scale(G_G2, p, k, l, o, n); }
int zkt_secp_scale_batch(const zkt_secp_affine* p, const uint64_t* k, int l, zkt_secp_affine* o, size_t n) { return group_scale(G_SECP, p, k, l, o, n); }
int zkt_g1_add_batch(const zkt_g1_affine* a, const zkt_g1_affine* b, zkt_g1_affine* o, size_t n) { return group_add(G_G1, a, b, o, n); }
int zkt_g2_add_batch(const zkt_g2_affine* a, const zkt_g2_affine* b, zkt_g2_affine* o, size_t n) { return group_add(G_G2, a, b, o, n); }
int zkt_secp_add_batch(const zkt_secp_affine* a, const zkt_secp_affine* b, zkt_secp_affine* o, size_t n) { return group_add(G_SECP, a, b, o, n); }
int zkt_g1_neg_batch(const zkt_g1_affine* a, zkt_g1_affine* o, size_t n) { return group_neg(G_G1, a, o, n); }
int zkt_g2_neg_batch(const zkt_g2_affine* a, zkt_g2_affine* o, size_t n) { return group_neg(G_G2, a, o, n); }
int zkt_g1_mul_batch(const zkt_g1_affine* p, const uint64_t* k, int l, zkt_g1_affine* o, size_t n) { return group_mul(G_G1, p, k, l, o, n); }
int zkt_g2_mul_batch(const zkt_g2_affine* p, const uint64_t* k, int l, zkt_g2_affine* o, size_t n) { return group_mul(G_G2, p, k, l, o, n); }
int zkt_secp_mul_batch(const zkt_secp_affine* p, const uint64_t* k, int l, zkt_secp_affine* o, size_t n) { return group_mul(G_SECP, p, k, l, o, n); }

// a16: is_rational_point / order-r membership / generators
static int group_pred(int grp, int pred, const void* pts, uint32_t* out, size_t n) {
  uint32_t order[8];                                                        // r (params.rs:14) or secp256k1's n
  for (int i = 0; i < 8; ++i) order[i] = grp == G_SECP ? SnC::mod32(i) : FrC::mod32(i);
  return staged(pts, abi_pt_bytes(grp), nullptr, 0, out, 4, n, ZKT_ERR_SHAPE,
                [&](uint32_t* da, uint32_t*, uint32_t* dout, hipStream_t s) -> hipError_t {
                  uint32_t* d_order = g.d_small;                           // g.mu is held by staged_raw
                  hipError_t e = hipMemcpyAsync(d_order, order, 32, hipMemcpyHostToDevice, s);
                  if (e != hipSuccess) return e;
                  return launch_group_pred(grp, pred, da, d_order, 8, dout, n, s);
                });
}
int zkt_g1_is_on_curve_batch(const zkt_g1_affine* p, uint32_t* out, size_t n) { return group_pred(G_G1, 0, p, out, n); }
int zkt_g2_is_on_curve_batch(const zkt_g2_affine* p, uint32_t* out, size_t n) { return group_pred(G_G2, 0, p, out, n); }
int zkt_secp_is_on_curve_batch(const zkt_secp_affine* p, uint32_t* out, size_t n) { return group_pred(G_SECP, 0, p, out, n); }
int zkt_g1_in_subgroup_batch(const zkt_g1_affine* p, uint32_t* out, size_t n) { return group_pred(G_G1, 1, p, out, n); }
int zkt_g2_in_subgroup_batch(const zkt_g2_affine* p, uint32_t* out, size_t n) { return group_pred(G_G2, 1, p, out, n); }
int zkt_secp_in_subgroup_batch(const zkt_secp_affine* p, uint32_t* out, size_t n) { return group_pred(G_SECP, 1, p, out, n); }
void zkt_g1_generator(zkt_g1_affine* out) { *out = G1_GEN; }
void zkt_g2_generator(zkt_g2_affine* out) { *out = G2_GEN; }
void zkt_secp_generator(zkt_secp_affine* out) { *out = SECP_GEN; }

int zkt_tate_batch(const zkt_g1_affine* g1, const zkt_g2_affine* g2, uint64_t* out, size_t n) {
  return staged(g1, sizeof(zkt_g1_affine), g2, sizeof(zkt_g2_affine), out, 576, n, ZKT_ERR_INFINITY,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_tate(da, db, dout, n, g.d_err, s); });
}
static int miller_exact(int which, const zkt_g1_affine* g1, const zkt_g2_affine* g2, uint64_t* out, size_t n) {
  return staged(g1, sizeof(zkt_g1_affine), g2, sizeof(zkt_g2_affine), out, 576, n, ZKT_ERR_INFINITY,
                [&](uint32_t* da, uint32_t* db, uint32_t* dout, hipStream_t s) { return launch_miller_exact(which, da, db, dout, n, g.d_err, s); });
}
int zkt_miller_g1g2_batch(const zkt_g1_affine* g1, const zkt_g2_affine* g2, uint64_t* out, size_t n) { return miller_exact(0, g1, g2, out, n); }
int zkt_miller_g2g1_batch(const zkt_g2_affine* g2, const zkt_g1_affine* g1, uint64_t* out, size_t n) { return miller_exact(1, g1, g2, out, n); }
int zkt_weil_batch(const zkt_g1_affine* g1, const zkt_g2_affine* g2, uint64_t* out, size_t n) { return miller_exact(2, g1, g2, out, n); }
int zkt_gt_eq(const uint64_t* a, const uint64_t* b) {
  if (!a || !b) return -ZKT_ERR_SHAPE;
  return memcmp(a, b, 576) == 0 ? 1 : 0;   // canonical residues: memcmp equality <=> Fq12 equality (fq12.rs:88-93)
}

// ---- device-resident entry points --------------------------------------------------
int zkt_fq_mul_batch_dev(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  HIPCHK(launch_fp_op(F_FQ, OP_MUL, (const uint32_t*)a, (const uint32_t*)b, (uint32_t*)out, n, g.d_err, (hipStream_t)stream));
  return ZKT_OK;
}
int zkt_g1_mul_batch_dev(const zkt_g1_affine* p, const uint64_t* k, int limbs, zkt_g1_affine* out, size_t n, void* stream) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (limbs < 1 || limbs > 6) return ZKT_ERR_SHAPE;
  HIPCHK(launch_group_mul(G_G1, (const uint32_t*)p, (const uint32_t*)k, limbs * 2, (uint32_t*)out, n, (hipStream_t)stream));
  return ZKT_OK;
}
int zkt_g2_mul_batch_dev(const zkt_g2_affine* p, const uint64_t* k, int limbs, zkt_g2_affine* out, size_t n, void* stream) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (limbs < 1 || limbs > 6) return ZKT_ERR_SHAPE;
  HIPCHK(launch_group_mul(G_G2, (const uint32_t*)p, (const uint32_t*)k, limbs * 2, (uint32_t*)out, n, (hipStream_t)stream));
  return ZKT_OK;
}
// The pairing kernels keep their Fq12 temporaries in 10-18 KB of scratch per lane, and the runtime sizes — and keeps — a queue's scratch for every wave slot
// of the device: 5-6 GiB per hardware queue that ever ran one (the process aborts when its pool is spent, at ~30 GB).  A caller with
// eight streams of its own would spend 8 x 6 GiB on them.  So the kernel never runs on the caller's stream: it runs on the library's ONE staging stream,
// ordered behind the caller's stream by an event (the inputs were produced there), and the call returns after the result is complete, so work the caller
// queues afterwards on ANY stream sees it.  tests/test_gpu_parity.py::test_tate_dev_from_many_caller_streams drives 8 streams through this.
// Three persistent events of the staging stream (created on first use under g.mu, released with the library's other device state): nothing is created or
// destroyed per call, and an early return leaks nothing.
static hipEvent_t g_tate_ev[3] = {nullptr, nullptr, nullptr};
static int tate_events() {
  if (g_tate_ev[0]) return ZKT_OK;
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  if (hipEventCreateWithFlags(&e[0], hipEventDisableTiming) != hipSuccess || hipEventCreate(&e[1]) != hipSuccess || hipEventCreate(&e[2]) != hipSuccess) {
    for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x);
    (void)hipGetLastError(); return ZKT_ERR_DEVICE;
  }
  for (int i = 0; i < 3; ++i) g_tate_ev[i] = e[i];
  return ZKT_OK;
}
static void tate_events_release() { for (hipEvent_t& x : g_tate_ev) { if (x) (void)hipEventDestroy(x); x = nullptr; } }
// BLOCKING, unlike the other *_dev entry points (include/zkt.h): the result is complete on return, and calls are serialised on the staging stream.
int zkt_tate_batch_dev(const zkt_g1_affine* g1, const zkt_g2_affine* g2, uint64_t* out, size_t n, void* stream) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  std::lock_guard<std::mutex> lk(g.mu);
  hipStream_t s = g.stream;
  int rc = tate_events(); if (rc) return rc;
  HIPCHK(hipEventRecord(g_tate_ev[0], (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(s, g_tate_ev[0], 0));
  rc = reset_err(s); if (rc) return rc;
  HIPCHK(hipEventRecord(g_tate_ev[1], s));
  HIPCHK(launch_tate((const uint32_t*)g1, (const uint32_t*)g2, (uint32_t*)out, n, g.d_err, s));
  HIPCHK(hipEventRecord(g_tate_ev[2], s));
  rc = fetch_err(s, ZKT_ERR_INFINITY);                  // synchronises the staging stream: the pairings are done when this returns
  HIPCHK(hipEventElapsedTime(&t_kernel_ms, g_tate_ev[1], g_tate_ev[2])); t_kernel_name = "k_tate";
  return rc;
}

// combine step of a sharded MSM: `count` Jacobian partials, `stride_words` u32 apart, summed by one wave and normalised
int zkt_internal_jac_sum(int grp, const uint32_t* dev_partials, size_t count, size_t stride_words, hipStream_t s, void* out) {
  if (!dev_partials || !out || count == 0) return ZKT_ERR_SHAPE;
  std::lock_guard<std::mutex> lk(g.mu);
  HIPCHK(launch_msm_jac_sum_to_affine(grp, dev_partials, count, stride_words, g.d_small, s));
  HIPCHK(hipMemcpyAsync(out, g.d_small, abi_pt_bytes(grp), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ZKT_OK;
}
static int jac_sum_dev(int grp, const uint32_t* dev_partials, size_t count, void* stream, void* out) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  return zkt_internal_jac_sum(grp, dev_partials, count, 3 * grp_coord_bytes(grp) / 4, (hipStream_t)stream, out);
}
// one-shot host-pointer MSM (eval_with_g1_hidings called once, polynomial.rs:271-281): the table-free form — upload, kernel layout,
// sort / accumulate / per-window reduce / join on one stream, free.  No window-multiple table is built for a single use.
static int msm_host(int grp, const void* bases, const uint64_t* scalars, size_t n, void* out) {
  if (ensure_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!out || (n && (!bases || !scalars)) || n >= (size_t(1) << 26)) return ZKT_ERR_SHAPE;      // entry offsets are 32-bit: nwin * n < 2^32
  if (n == 0) { set_infinity(out, abi_pt_bytes(grp)); return ZKT_OK; }
  const MsmPlan plan = msm_plan_direct(n, grp);
  const size_t ptb = abi_pt_bytes(grp), cb = grp_coord_bytes(grp);
  const size_t o_abi = 0, o_sc = padded(n * ptb), o_tab = o_sc + padded(n * 32), o_inf = o_tab + padded(n * 2 * cb), o_jac = o_inf + padded(n),
               o_out = o_jac + padded(4 * cb), o_ws = o_out + padded(ptb), total = o_ws + plan.ws_bytes;
  Dev buf;                                                   // [abi points | scalars | kernel-layout points | inf flags | jac | abi out | workspace]
  ZCHK(buf.alloc(total));
  uint8_t* const blob = (uint8_t*)buf.p;
  if (debug_poison()) { HIPCHK(hipMemset(blob, 0xA5, total)); HIPCHK(hipDeviceSynchronize()); }
  std::lock_guard<std::mutex> lk(g.mu);                      // g.stream is the library's staging stream
  hipStream_t s = g.stream;
  int rc = ZKT_OK;
  auto fail = [&](hipError_t e) { if (e != hipSuccess) { fprintf(stderr, "[zkt] HIP error %s in one-shot MSM\n", hipGetErrorString(e)); rc = ZKT_ERR_DEVICE; } return e != hipSuccess; };
  if (!fail(hipMemcpyAsync(blob + o_abi, bases, n * ptb, hipMemcpyHostToDevice, s)) && !fail(hipMemcpyAsync(blob + o_sc, scalars, n * 32, hipMemcpyHostToDevice, s)) &&
      !fail(launch_msm_to_kernel_layout(grp, (const uint32_t*)(blob + o_abi), (uint32_t*)(blob + o_tab), blob + o_inf, n, s)) &&
      !fail(launch_msm_sort(plan, blob + o_inf, (const uint32_t*)(blob + o_sc), blob + o_ws, s)) &&
      !fail(launch_msm_accumulate(plan, (const uint32_t*)(blob + o_tab), blob + o_ws, s)) &&
      !fail(launch_msm_reduce(plan, blob + o_ws, (uint32_t*)(blob + o_jac), (uint32_t*)(blob + o_out), s)) &&
      !fail(hipMemcpyAsync(out, blob + o_out, ptb, hipMemcpyDeviceToHost, s)))
    fail(hipStreamSynchronize(s));
  else (void)hipStreamSynchronize(s);                       // either way nothing is queued on the buffer when it goes
  return rc;
}


#define ZKT_MSM_STAGED_API(NAME, GRP, PT)                                                                                       \
  int zkt_##NAME##_jac_sum_dev(const uint32_t* partials, size_t count, void* stream, PT* out) { return jac_sum_dev(GRP, partials, count, stream, out); } \
  int zkt_##NAME##_msm(const PT* bases, const uint64_t* scalars, size_t n, PT* out) { return msm_host(GRP, bases, scalars, n, out); }
ZKT_MSM_STAGED_API(g1, G_G1, zkt_g1_affine)
ZKT_MSM_STAGED_API(g2, G_G2, zkt_g2_affine)
ZKT_MSM_STAGED_API(secp, G_SECP, zkt_secp_affine)

}  // extern "C"
