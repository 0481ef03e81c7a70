// SHA-256 (FIPS 180-4) as inline host/device math: one message per caller, i.e. per lane on the device.
//   Sha256 / get_digest          src/building_block/hasher/sha256.rs:34-86 (K :48-59, initial hash value :61-72, to_u8_array :10-22)
//   pad_msg / compute_hash       src/building_block/hasher/sha_common.rs:157-186 (0x80, zeros up to 56 mod 64, the bit length as 8 big-endian bytes)
// The message schedule is a rolling window of 16 words (W[t] overwrites W[t-16]), all indices compile-time constants, so it stays in registers.
// A message runs serially on its caller: a long message is one lane's work however many lanes the launch has (65 rounds-of-64 per KiB); the batch
// kernels get their parallelism from the number of messages, which is what signature batches provide.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkt_constants.h"

namespace zkt {

// the round constants: constant memory on the device (every lane reads the same word in the same round: a scalar load), a plain table on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define ZKT_SHA_CONST __constant__ static const
#else
#define ZKT_SHA_CONST static const
#endif
ZKT_SHA_CONST uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
#undef ZKT_SHA_CONST

ZKT_HD uint32_t sha_rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

ZKT_HD void sha256_init(uint32_t h[8]) {                                                  // sha256.rs:61-72
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// one block: w holds its sixteen big-endian words on entry and is used up as the schedule window (compute_hash, sha_common.rs)
ZKT_HD void sha256_compress(uint32_t h[8], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
  for (int t0 = 0; t0 < 64; t0 += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (t0) {                                                                           // W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16], in place
        const uint32_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
        const uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
        const uint32_t s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
        w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
      }
      const uint32_t S1 = sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25);
      const uint32_t ch = (e & f) ^ (~e & g);
      const uint32_t t1 = hh + S1 + ch + SHA256_K[t0 + j] + w[j];
      const uint32_t S0 = sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22);
      const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint32_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// byte `pos` of the padded message (pad_msg, sha_common.rs:157-186): the message, 0x80, zeros, and the bit length in the last eight bytes
ZKT_HD uint32_t sha256_padded_byte(const uint8_t* msg, uint64_t len, uint64_t padded_len, uint64_t pos) {
  if (pos < len) return msg[pos];
  if (pos == len) return 0x80u;
  if (pos + 8 < padded_len) return 0u;
  return (uint32_t)(((len << 3) >> (8 * (padded_len - 1 - pos))) & 0xffu);
}

// h = the eight state words of SHA-256(msg[0..len)); the digest bytes are these words big-endian (to_u8_array, sha256.rs:10-22).
// msg may start at any byte address: a block that lies wholly inside the message and starts on a 4-byte boundary is read as sixteen words, every
// other block (unaligned starts, and the one or two blocks that hold the padding) byte by byte.
ZKT_HD void sha256_words(const uint8_t* msg, uint64_t len, uint32_t h[8]) {
  const uint64_t padded_len = ((len + 8) / 64 + 1) * 64;                                 // len + 1 + 8 rounded up to a block: 55 -> 64, 56 -> 128
  sha256_init(h);
  const bool aligned = (((uintptr_t)msg) & 3u) == 0;
  for (uint64_t base = 0; base < padded_len; base += 64) {
    uint32_t w[16];
    if (aligned && base + 64 <= len) {
      const uint32_t* p = (const uint32_t*)(msg + base);
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = __builtin_bswap32(p[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint64_t q = base + 4 * (uint64_t)j;
        w[j] = (sha256_padded_byte(msg, len, padded_len, q) << 24) | (sha256_padded_byte(msg, len, padded_len, q + 1) << 16) |
               (sha256_padded_byte(msg, len, padded_len, q + 2) << 8) | sha256_padded_byte(msg, len, padded_len, q + 3);
      }
    }
    sha256_compress(h, w);
  }
}
ZKT_HD void sha256_store_digest(const uint32_t h[8], uint8_t* out) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
}

}  // namespace zkt
