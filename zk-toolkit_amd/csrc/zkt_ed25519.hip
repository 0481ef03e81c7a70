// Batched SHA-512 and Ed25519: one message / one key / one signature per lane, one launch per call.
//   Sha512::get_digest           src/building_block/hasher/sha512.rs:91-97
//   Ed25519Sha512::decode_point  src/building_block/curves/curve25519/ed25519_sha512.rs:85-98
//   gen_pub_key / sign / verify  ed25519_sha512.rs:115-125, :127-158, :160-186
// The math is sha512.h, fe25519.h and ed25519.h (host/device inline, checked on the host by csrc/hostcheck.cpp); this file holds the kernels, their
// launchers and the base point's comb table.  A lane hashes what it signs or verifies itself: no digest leaves the registers.
#include <mutex>
#include "ed25519.h"
#include "zkt_internal.h"

namespace zkt {

__device__ __forceinline__ uint64_t ed_msg_len(const unsigned long long* off, size_t i) { return off[i + 1] > off[i] ? off[i + 1] - off[i] : 0; }

__global__ void __launch_bounds__(64) k_sha512(const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off, size_t n, uint8_t* __restrict__ digests) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t h[8];
  sha512_words<0>(nullptr, msgs + off[i], ed_msg_len(off, i), h);
  uint64_t* out = (uint64_t*)(digests + i * 64);               // the library's own buffer, 64 bytes per element: word stores, big-endian words as to_u8_array writes them
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = __builtin_bswap64(h[j]);
}

__global__ void __launch_bounds__(64) k_ed25519_table(uint32_t* __restrict__ table) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ED_COMB_ENTRIES) return;
  ed25519_comb_entry(t, table + (size_t)t * ED_PRE_WORDS);
}

// xy[i] = {x, y} canonical (8 + 8 words), on_curve[i] = 1/0
__global__ void __launch_bounds__(64) k_ed25519_decode(const uint8_t* __restrict__ enc, size_t n, uint32_t* __restrict__ xy, uint32_t* __restrict__ on_curve) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8], o[8]; Fe x, y;
  ld_le_words(enc + i * 32, w, 8);
  on_curve[i] = ed25519_decode_one(w, x, y) ? 1u : 0u;
  fe_to_words(x, o);
#pragma unroll
  for (int j = 0; j < 8; ++j) xy[i * 16 + j] = o[j];
  fe_to_words(y, o);
#pragma unroll
  for (int j = 0; j < 8; ++j) xy[i * 16 + 8 + j] = o[j];
}

__global__ void __launch_bounds__(64) k_ed25519_public_keys(const uint8_t* __restrict__ prv, const uint32_t* __restrict__ btab, size_t n, uint8_t* __restrict__ pub) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed25519_public_key_one(prv + i * 32, btab, pub + i * 32);
}

__global__ void __launch_bounds__(64) k_ed25519_sign(const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off, const uint8_t* __restrict__ prv,
                                                     const uint32_t* __restrict__ btab, size_t n, uint8_t* __restrict__ sigs) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  ed25519_sign_one(msgs + off[i], ed_msg_len(off, i), prv + i * 32, btab, sigs + i * 64);
}

// The table of the key's multiples is the lane's frame: ED_TAB cached entries of 128 bytes (1,920 bytes at the 4-bit width), read with a run-time index
// once per window.  -DZKT_ED25519_TABLE_LDS (an A/B build of tools/diag/ed25519_timing.py, not shipped) puts it in LDS instead, the 64 lanes interleaved
// word by word: 122,880 bytes per block at 4 bits, i.e. one wave per CU; 57,344 bytes at 3 bits (-DZKT_ED25519_WIN=3).
// -DZKT_ED25519_WAVES=w asks the register allocator for w waves per SIMD (512 / w registers per lane).  Shipped with w = 2 (Makefile): 256 registers, 33 spilled;
// left alone the allocator takes 287 and ONE wave runs per SIMD (8.2 against 6.0 ms per 2^18 signatures, profiles/ed25519_timing.md).
#if defined(ZKT_ED25519_WAVES)
#define ZKT_ED25519_VERIFY_ATTR __attribute__((amdgpu_waves_per_eu(ZKT_ED25519_WAVES, ZKT_ED25519_WAVES)))
#else
#define ZKT_ED25519_VERIFY_ATTR
#endif
__global__ void __launch_bounds__(64) ZKT_ED25519_VERIFY_ATTR k_ed25519_verify(const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off, const uint8_t* __restrict__ sigs,
                                                       const uint8_t* __restrict__ pub, const uint32_t* __restrict__ btab, size_t n, uint32_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
#if defined(ZKT_ED25519_TABLE_LDS)
  __shared__ uint32_t lds_tab[ED_TAB * ED_CW * 64];
  ok[i] = ed25519_verify_one<64>(msgs + off[i], ed_msg_len(off, i), sigs + i * 64, pub + i * 32, btab, lds_tab + threadIdx.x) ? 1u : 0u;
#else
  uint32_t tab[ED_TAB * ED_CW];
  ok[i] = ed25519_verify_one<1>(msgs + off[i], ed_msg_len(off, i), sigs + i * 64, pub + i * 32, btab, tab) ? 1u : 0u;
#endif
}

// ---- the comb table of B: built on the first Ed25519 call of a process, released by zkt_shutdown ---------------------------------------------------
namespace {
struct BaseTable { std::mutex mu; uint32_t* dev = nullptr; };
BaseTable g_ed_table;
}
void ed25519_release_device_state() {
  std::lock_guard<std::mutex> lk(g_ed_table.mu);
  if (g_ed_table.dev) { (void)hipFree(g_ed_table.dev); g_ed_table.dev = nullptr; }
}
hipError_t ed25519_base_table(const uint32_t** table, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_ed_table.mu);
  if (!g_ed_table.dev) {                                         // first use in this process: build on the caller's stream and wait, so that later callers on other streams find it complete
    uint32_t* mem = nullptr; hipError_t e;
    if ((e = hipMalloc((void**)&mem, (size_t)ED_COMB_ENTRIES * ED_PRE_WORDS * 4)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ed25519_table, dim3(ED_COMB_ENTRIES / 64), dim3(64), 0, s, mem);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) { (void)hipFree(mem); return e; }
    g_ed_table.dev = mem;
  }
  *table = g_ed_table.dev;
  return hipSuccess;
}

hipError_t launch_sha512(const uint8_t* msgs, const unsigned long long* off, size_t n, uint8_t* digests, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha512, dim3(grid_blocks(n, 64)), dim3(64), 0, s, msgs, off, n, digests);
  return hipGetLastError();
}
hipError_t launch_ed25519_decode(const uint8_t* enc, size_t n, uint32_t* xy, uint32_t* on_curve, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ed25519_decode, dim3(grid_blocks(n, 64)), dim3(64), 0, s, enc, n, xy, on_curve);
  return hipGetLastError();
}
hipError_t launch_ed25519_public_keys(const uint8_t* prv, const uint32_t* btab, size_t n, uint8_t* pub, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!btab) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ed25519_public_keys, dim3(grid_blocks(n, 64)), dim3(64), 0, s, prv, btab, n, pub);
  return hipGetLastError();
}
hipError_t launch_ed25519_sign(const uint8_t* msgs, const unsigned long long* off, const uint8_t* prv, const uint32_t* btab, size_t n, uint8_t* sigs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!btab || !off) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ed25519_sign, dim3(grid_blocks(n, 64)), dim3(64), 0, s, msgs, off, prv, btab, n, sigs);
  return hipGetLastError();
}
hipError_t launch_ed25519_verify(const uint8_t* msgs, const unsigned long long* off, const uint8_t* sigs, const uint8_t* pub, const uint32_t* btab, size_t n, uint32_t* ok,
                                 hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!btab || !off) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ed25519_verify, dim3(grid_blocks(n, 64)), dim3(64), 0, s, msgs, off, sigs, pub, btab, n, ok);
  return hipGetLastError();
}

}  // namespace zkt
