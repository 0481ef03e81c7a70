// SHA-512 (FIPS 180-4) as inline host/device math: one message per caller, i.e. per lane on the device.
//   Sha512 / get_digest          src/building_block/hasher/sha512.rs:37-102 (K :52-75, initial hash value :77-88, to_u8_array :10-26)
//   pad_msg / compute_hash       src/building_block/hasher/sha_common.rs:157-186 (0x80, zeros up to 112 mod 128, the bit length in the last 16 bytes)
// The hashed string is `prefix ‖ msg`: a prefix of 0, 32 or 64 bytes that the caller holds in registers as big-endian 64-bit words, followed by the
// message in memory.  Ed25519 hashes prefix‖msg and R‖A‖msg (ed25519_sha512.rs:139-152, :170-174); neither string is ever assembled in memory.
// The schedule is a rolling window of 16 words with compile-time indices, as in sha256.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkt_constants.h"

namespace zkt {

#if defined(__HIP_DEVICE_COMPILE__)
#define ZKT_SHA_CONST __constant__ static const
#else
#define ZKT_SHA_CONST static const
#endif
ZKT_SHA_CONST uint64_t SHA512_K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull,
    0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull,
    0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull,
    0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
    0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull,
    0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull, 0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull,
    0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
    0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull,
    0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
#undef ZKT_SHA_CONST

ZKT_HD uint64_t sha_rotr64(uint64_t x, int r) { return (x >> r) | (x << (64 - r)); }

ZKT_HD void sha512_init(uint64_t h[8]) {                                                  // sha512.rs:77-88
  h[0] = 0x6a09e667f3bcc908ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull; h[3] = 0xa54ff53a5f1d36f1ull;
  h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full; h[6] = 0x1f83d9abfb41bd6bull; h[7] = 0x5be0cd19137e2179ull;
}

// one block: w holds its sixteen big-endian words on entry and is used up as the schedule window (compute_hash, sha_common.rs; the rotation counts are sha512.rs:44-47)
ZKT_HD void sha512_compress(uint64_t h[8], uint64_t w[16]) {
  uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
  for (int t0 = 0; t0 < 80; t0 += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (t0) {                                                                           // W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16], in place
        const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
        const uint64_t s0 = sha_rotr64(w15, 1) ^ sha_rotr64(w15, 8) ^ (w15 >> 7);
        const uint64_t s1 = sha_rotr64(w2, 19) ^ sha_rotr64(w2, 61) ^ (w2 >> 6);
        w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
      }
      const uint64_t S1 = sha_rotr64(e, 14) ^ sha_rotr64(e, 18) ^ sha_rotr64(e, 41);
      const uint64_t ch = (e & f) ^ (~e & g);
      const uint64_t t1 = hh + S1 + ch + SHA512_K[t0 + j] + w[j];
      const uint64_t S0 = sha_rotr64(a, 28) ^ sha_rotr64(a, 34) ^ sha_rotr64(a, 39);
      const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint64_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// length of the padded string: len + 1 + 16 rounded up to a block (111 -> 128, 112 -> 256)
ZKT_HD uint64_t sha512_padded_len(uint64_t len) { return ((len + 16) / 128 + 1) * 128; }

// byte `pos` of the padded MESSAGE PART (pad_msg, sha_common.rs:157-186), positions counted from the start of prefix‖msg: pos >= plen.
// total = plen + len.  The message, 0x80, zeros, and the bit length of the whole string in the last sixteen bytes.
ZKT_HD uint32_t sha512_padded_byte(const uint8_t* msg, uint64_t plen, uint64_t total, uint64_t padded_len, uint64_t pos) {
  if (pos < total) return msg[pos - plen];
  if (pos == total) return 0x80u;
  if (pos + 16 < padded_len) return 0u;
  const uint64_t k = padded_len - 1 - pos;                                                // 0 = the last byte
  return (uint32_t)((k < 8 ? (total << 3) >> (8 * k) : (total >> 61) >> (8 * (k - 8))) & 0xffu);
}

// h = the eight state words of SHA-512(prefix ‖ msg[0..len)); the digest bytes are these words big-endian (to_u8_array, sha512.rs:10-26).
// PW = 0, 4 or 8 prefix words (pre[j] = bytes 8j .. 8j+7 of the prefix, big-endian).  msg may start at any byte address: a word that lies wholly inside
// the message and on an 8-byte boundary is one 64-bit load, every other word (unaligned starts, the words that hold padding) is read byte by byte.
template <int PW> ZKT_HD void sha512_words(const uint64_t* pre, const uint8_t* msg, uint64_t len, uint64_t h[8]) {
  constexpr uint64_t plen = 8 * (uint64_t)PW;
  const uint64_t total = plen + len, padded_len = sha512_padded_len(total);
  sha512_init(h);
  const bool aligned = ((((uintptr_t)msg) & 7u) == 0);                                    // plen is a multiple of 8: string position and address are aligned together
  for (uint64_t base = 0; base < padded_len; base += 128) {
    uint64_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t q = base + 8 * (uint64_t)j;
      if (j < PW && base == 0) { w[j] = pre[j < PW ? j : 0]; continue; }
      if (aligned && q + 8 <= total) { w[j] = __builtin_bswap64(*(const uint64_t*)(msg + (q - plen))); continue; }
      uint64_t v = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) v = (v << 8) | sha512_padded_byte(msg, plen, total, padded_len, q + b);
      w[j] = v;
    }
    sha512_compress(h, w);
  }
}
ZKT_HD void sha512_store_digest(const uint64_t h[8], uint8_t* out) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(h[i] >> (56 - 8 * b));
  }
}

}  // namespace zkt
