// Host-side plumbing shared by the translation units that implement the C ABI (the .cpp files, and the .hip files that hold entry points of include/zkt.h):
// the HIP-error check, an owning device buffer, the end of a verdict call, the ABI point sizes and the generators.
// Host code only: no device header includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <cstdio>
#include <cstdlib>
#include "../../include/zkt.h"
#include "zkt_internal.h"

// a failed HIP call: report it, clear the runtime's last error (a launcher that ends in hipGetLastError must not see it later), return ZKT_ERR_DEVICE
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[zkt] HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); return ZKT_ERR_DEVICE; } } while (0)
// a failed library call: pass its status on
#define ZCHK(x) do { int _rc = (x); if (_rc != ZKT_OK) return _rc; } while (0)

namespace zkt {
namespace {                         // internal linkage in every translation unit: nothing here is exported from the library

// Owning device buffer; p is null when the allocation failed.  pooled: stream-ordered on the legacy stream (hipMallocAsync / hipFreeAsync) — for the
// per-call buffers of the verification entry points, which run entirely on that stream: a dozen hipMalloc (33-72 us each) and the device-wide wait
// inside every hipFree were ~0.6 ms of a 4.9 ms verification.
struct Dev {
  void* p = nullptr;
  uint64_t pooled = 0;              // a word, not a bool: without padding, the constructor of a handle that holds many buffers (zkt_groth16_pk) stays inline, not exported
  Dev() = default;
  explicit Dev(size_t bytes, bool pool = false) { alloc(bytes, pool); }
  ~Dev() { release(); }
  int alloc(size_t bytes, bool pool = false) {
    pooled = pool;
    const size_t b = bytes ? bytes : 32;
    if ((pooled ? hipMallocAsync(&p, b, nullptr) : hipMalloc(&p, b)) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return ZKT_ERR_DEVICE; }
    return ZKT_OK;
  }
  void release() { if (p) { if (pooled) (void)hipFreeAsync(p, nullptr); else (void)hipFree(p); } p = nullptr; }
  uint32_t* w() const { return (uint32_t*)p; }
  Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
};
// host -> the buffer's start, and device -> host, queued on s
inline int up(Dev& d, const void* h, size_t bytes, hipStream_t s) { if (!d.p) return ZKT_ERR_DEVICE; if (bytes) HIPCHK(hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, s)); return ZKT_OK; }
inline int down(void* h, const void* d, size_t bytes, hipStream_t s) { if (bytes) HIPCHK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s)); return ZKT_OK; }
// The end of a call whose kernels wrote n verdicts at dok and the index of the first offending element (or NO_ERR) at derr: both come down, s is waited for,
// and a recorded index is reported (zkt_last_error_index) with `status`.  ok == nullptr: the error word alone.  Allocates nothing.
inline int finish_verdicts(uint32_t* ok, const void* dok, size_t n, const void* derr, hipStream_t s, int status = ZKT_ERR_INFINITY) {
  unsigned long long e = NO_ERR; int rc;
  if ((ok && (rc = down(ok, dok, n * 4, s))) || (rc = down(&e, derr, 8, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  if (e != NO_ERR) { zkt_internal_set_error_index((size_t)e); return status; }
  return ZKT_OK;
}

// ABI sizes (include/zkt.h)
constexpr size_t G1B = sizeof(zkt_g1_affine), G2B = sizeof(zkt_g2_affine), SPB = sizeof(zkt_secp_affine), FRB = 32;
inline size_t abi_pt_bytes(int grp) { return grp == G_G1 ? G1B : grp == G_G2 ? G2B : SPB; }
// one internal (Montgomery) coordinate of a group's points: a third of a Jacobian partial (zkt_api.cpp asserts ZKT_*_PARTIAL_WORDS against the limb layout)
inline size_t grp_coord_bytes(int grp) { return 4 * (grp == G_G1 ? ZKT_G1_PARTIAL_WORDS : grp == G_G2 ? ZKT_G2_PARTIAL_WORDS : ZKT_SECP_PARTIAL_WORDS) / 3; }
// ZKT_DEBUG_POISON=1: every MSM workspace is filled with a garbage pattern when it is allocated, so a kernel that reads a word nobody wrote gets 0xA5A5A5A5
// instead of the zeros a fresh allocation happens to hold (tools/diag/msm_repeat.py and the MSM tests are run this way).
inline bool debug_poison() { static const bool on = [] { const char* e = getenv("ZKT_DEBUG_POISON"); return e && *e == '1'; }(); return on; }

// a 4-limb value that is 0 mod r: 0, r or 2r (3r > 2^256).  Values are reduced on load, so a trapdoor must pass this test, not a test of its raw limbs.
inline bool fr_is_zero_mod_r(const uint64_t* a) {
  constexpr uint64_t r[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
  uint64_t m[4] = {0, 0, 0, 0};                     // 0, then r, then 2r
  for (int k = 0; k < 3; ++k) {
    if (a[0] == m[0] && a[1] == m[1] && a[2] == m[2] && a[3] == m[3]) return true;
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; ++j) { c += (unsigned __int128)m[j] + r[j]; m[j] = (uint64_t)c; c >>= 64; }
  }
  return false;
}

// The standard generators in the ABI layout (canonical coordinates, little-endian u64 limbs)
constexpr zkt_g1_affine G1_GEN = {                                            // g1_point.rs:38-47
    {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull},
    {0x0caa232946c5e7e1ull, 0xd03cc744a2888ae4ull, 0x00db18cb2c04b3edull, 0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x08b3f481e3aaa0f1ull}, 0, 0};
constexpr zkt_g2_affine G2_GEN = {                                            // g2_point.rs:36-46; Fq2 = {u1, u0}
    {0xe5ac7d055d042b7eull, 0x334cf11213945d57ull, 0xb5da61bbdc7f5049ull, 0x596bd0d09920b61aull, 0x7dacd3a088274f65ull, 0x13e02b6052719f60ull,
     0xd48056c8c121bdb8ull, 0x0bac0326a805bbefull, 0xb4510b647ae3d177ull, 0xc6e47ad4fa403b02ull, 0x260805272dc51051ull, 0x024aa2b2f08f0a91ull},
    {0xaaa9075ff05f79beull, 0x3f370d275cec1da1ull, 0x267492ab572e99abull, 0xcb3e287e85a763afull, 0x32acd2b02bc28b99ull, 0x0606c4a02ea734ccull,
     0xe193548608b82801ull, 0x923ac9cc3baca289ull, 0x6d429a695160d12cull, 0xadfd9baa8cbdd3a7ull, 0x8cc9cdc6da2e351aull, 0x0ce5d527727d6e11ull}, 0, 0};
constexpr zkt_secp_affine SECP_GEN = {                                        // secp256k1/affine_point.rs:40-47
    {0x59f2815b16f81798ull, 0x029bfcdb2dce28d9ull, 0x55a06295ce870b07ull, 0x79be667ef9dcbbacull},
    {0x9c47d08ffb10d4b8ull, 0xfd17b448a6855419ull, 0x5da4fbfc0e1108a8ull, 0x483ada7726a3c465ull}, 0, 0};

}  // namespace
}  // namespace zkt
