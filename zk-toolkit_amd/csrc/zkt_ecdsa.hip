// Batched SHA-256 and secp256k1 ECDSA: one message / one signature per lane, one launch per call.
//   Sha256::get_digest   src/building_block/hasher/sha256.rs:75-81
//   Ecdsa::sign          src/building_block/curves/secp256k1/ecdsa.rs:37-85
//   Ecdsa::verify        ecdsa.rs:88-135
// The math is sha256.h and ecdsa.h (host/device inline, checked on the host by csrc/hostcheck.cpp); this file holds the kernels and their launchers.
// The message forms hash on the lane that then signs or verifies: the digest never leaves the registers.
#include "ecdsa.h"
#include "zkt_internal.h"

namespace zkt {

// an element whose end lies before its start is an empty message (as the BLS hash kernel's loop treats it): no byte of it is read
__device__ __forceinline__ uint64_t msg_len(const unsigned long long* off, size_t i) { return off[i + 1] > off[i] ? off[i + 1] - off[i] : 0; }

__global__ void __launch_bounds__(64) k_sha256(const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off, size_t n, uint8_t* __restrict__ digests) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t h[8];
  sha256_words(msgs + off[i], msg_len(off, i), h);
  uint32_t* out = (uint32_t*)(digests + i * 32);               // hipMalloc'ed and 32 bytes per element: word stores, big-endian words as to_u8_array writes them
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = __builtin_bswap32(h[j]);
}

// z of element i: from its digest, or from its message hashed here
__device__ __forceinline__ void ecdsa_load_z(const uint8_t* digests, const uint8_t* msgs, const unsigned long long* off, size_t i, uint32_t z[8]) {
  if (digests) { ecdsa_z_from_digest(digests + i * 32, z); return; }
  uint32_t h[8];
  sha256_words(msgs + off[i], msg_len(off, i), h);
  ecdsa_z_from_state(h, z);
}

// The table of the public key's multiples is the lane's frame: ECDSA_TAB Jacobian entries of 96 bytes (1,440 bytes at the 4-bit width), read with a
// run-time index once per window.  -DZKT_ECDSA_TABLE_LDS (an A/B build of tools/diag/ecdsa_timing.py, not shipped) puts it in LDS instead, the 64 lanes
// interleaved word by word: 92,160 bytes per block at 4 bits — gfx950 lets one block declare all 160 KiB of a CU's LDS, but then ONE wave runs per CU —
// and 43,008 bytes at 3 bits (three blocks per CU), against the sixteen waves per CU that 127 VGPRs allow with the table in the frame.
// profiles/ecdsa_timing.md has the rows.
__global__ void __launch_bounds__(64) k_ecdsa_verify(const uint8_t* __restrict__ digests, const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off,
                                                     const uint32_t* __restrict__ sigs, const uint32_t* __restrict__ pks, const uint32_t* __restrict__ gtab,
                                                     uint32_t* __restrict__ ok, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t z[8], r[8], s[8];
  ecdsa_load_z(digests, msgs, off, i, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) { r[j] = sigs[i * 16 + j]; s[j] = sigs[i * 16 + 8 + j]; }
#if defined(ZKT_ECDSA_TABLE_LDS)
  __shared__ uint32_t lds_tab[ECDSA_TAB * ECDSA_JW * 64];
  ok[i] = ecdsa_verify_one<64>(z, r, s, pks + i * ABI_SECP_WORDS, gtab, lds_tab + threadIdx.x) ? 1u : 0u;
#else
  uint32_t tab[ECDSA_TAB * ECDSA_JW];
  ok[i] = ecdsa_verify_one<1>(z, r, s, pks + i * ABI_SECP_WORDS, gtab, tab) ? 1u : 0u;
#endif
}

__global__ void __launch_bounds__(64) k_ecdsa_sign(const uint8_t* __restrict__ digests, const uint8_t* __restrict__ msgs, const unsigned long long* __restrict__ off,
                                                   const uint32_t* __restrict__ sks, const uint32_t* __restrict__ ks, const uint32_t* __restrict__ gtab,
                                                   uint32_t* __restrict__ sigs, uint32_t* __restrict__ retry, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t z[8], d[8], k[8], r[8], s[8];
  ecdsa_load_z(digests, msgs, off, i, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) { d[j] = sks[i * 8 + j]; k[j] = ks[i * 8 + j]; }
  retry[i] = ecdsa_sign_one(z, d, k, gtab, r, s) ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) { sigs[i * 16 + j] = r[j]; sigs[i * 16 + 8 + j] = s[j]; }
}

hipError_t launch_sha256(const uint8_t* msgs, const unsigned long long* off, size_t n, uint8_t* digests, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha256, dim3(grid_blocks(n, 64)), dim3(64), 0, s, msgs, off, n, digests);
  return hipGetLastError();
}
hipError_t launch_ecdsa_verify(const uint8_t* digests, const uint8_t* msgs, const unsigned long long* off, const uint32_t* sigs, const uint32_t* pks,
                               const uint32_t* gtab, uint32_t* ok, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!gtab || (!digests && !off)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ecdsa_verify, dim3(grid_blocks(n, 64)), dim3(64), 0, s, digests, msgs, off, sigs, pks, gtab, ok, n);
  return hipGetLastError();
}
hipError_t launch_ecdsa_sign(const uint8_t* digests, const uint8_t* msgs, const unsigned long long* off, const uint32_t* sks, const uint32_t* ks,
                             const uint32_t* gtab, uint32_t* sigs, uint32_t* retry, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!gtab || (!digests && !off)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ecdsa_sign, dim3(grid_blocks(n, 64)), dim3(64), 0, s, digests, msgs, off, sks, ks, gtab, sigs, retry, n);
  return hipGetLastError();
}

}  // namespace zkt
