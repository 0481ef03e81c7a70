// C ABI (include/zkt.h) of the hashes and signatures: SHA-256 and secp256k1 ECDSA (zkt_ecdsa.hip), SHA-512 and Ed25519 (zkt_ed25519.hip).
// Host-pointer calls stage through the library's arena on its staging stream, one Stage (host_stage.h) per call; the two `_dev` calls launch on the
// caller's stream.  The arena, the lock and the 4 KB of one-point scratch are reached through Stage only, the rest through the zkt_internal_* hooks.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/zkt.h"
#include "zkt_internal.h"
#include "host_abi.h"
#include "host_stage.h"

using namespace zkt;

namespace {

// the secp256k1 generator's comb table (built on first use, from a device copy of the generator in the one-point scratch, which `st` holds the lock for)
int secp_generator_table(const Stage& st, hipStream_t s, const uint32_t** table) {
  hipError_t e = generator_table(G_SECP, nullptr, table, s);
  if (e == hipErrorNotReady) {
    HIPCHK(hipMemcpyAsync(st.small(), &SECP_GEN, SPB, hipMemcpyHostToDevice, s));
    e = generator_table(G_SECP, st.small(), table, s);
  }
  HIPCHK(e);
  return ZKT_OK;
}
// what an ECDSA call hashes: the digests, or the messages with their offsets (the lane hashes its own first)
struct EcdsaInput { int dig = Stage::NONE, msgs = Stage::NONE, off = Stage::NONE; };
int ecdsa_input(Stage& st, const uint8_t* digests, const uint8_t* msgs, const uint64_t* offsets, size_t n, EcdsaInput& in) {
  if (digests) { in.dig = st.in(digests, n * 32); return ZKT_OK; }
  return st.msgs(msgs, offsets, n, in.msgs, in.off);
}
int ecdsa_verify_host(const uint8_t* digests, const uint8_t* msgs, const uint64_t* offsets, const zkt_ecdsa_sig* sigs, const zkt_secp_affine* pks, size_t n, uint32_t* ok) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!sigs || !pks || !ok || (digests ? false : (!offsets || (offsets[n] && !msgs)))) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; EcdsaInput in; const uint32_t* gtab = nullptr;
  ZCHK(secp_generator_table(st, st.stream(), &gtab));
  ZCHK(ecdsa_input(st, digests, msgs, offsets, n, in));
  const int is = st.in(sigs, n * sizeof(zkt_ecdsa_sig)), ip = st.in(pks, n * SPB), io = st.out(ok, n * 4);
  ZCHK(st.commit());
  HIPCHK(launch_ecdsa_verify(st.ptr<uint8_t>(in.dig), st.ptr<uint8_t>(in.msgs), st.ptr<unsigned long long>(in.off), st.ptr<uint32_t>(is), st.ptr<uint32_t>(ip), gtab,
                             st.ptr<uint32_t>(io), n, st.stream()));
  return st.finish();
}
int ecdsa_sign_host(const uint8_t* digests, const uint8_t* msgs, const uint64_t* offsets, const uint64_t* sks, const uint64_t* ks, size_t n, zkt_ecdsa_sig* sigs, uint32_t* retry) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!sks || !ks || !sigs || (digests ? false : (!offsets || (offsets[n] && !msgs)))) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  std::vector<uint32_t> own;                                   // a null `retry` is allowed when no element needs one: the flags are still read back
  if (!retry) { own.resize(n); }
  uint32_t* flags = retry ? retry : own.data();
  Stage st; EcdsaInput in; const uint32_t* gtab = nullptr;
  ZCHK(secp_generator_table(st, st.stream(), &gtab));
  ZCHK(ecdsa_input(st, digests, msgs, offsets, n, in));
  const int isk = st.in(sks, n * FRB), ik = st.in(ks, n * FRB), is = st.out(sigs, n * sizeof(zkt_ecdsa_sig)), ifl = st.out(flags, n * 4);
  ZCHK(st.commit());
  HIPCHK(launch_ecdsa_sign(st.ptr<uint8_t>(in.dig), st.ptr<uint8_t>(in.msgs), st.ptr<unsigned long long>(in.off), st.ptr<uint32_t>(isk), st.ptr<uint32_t>(ik), gtab,
                           st.ptr<uint32_t>(is), st.ptr<uint32_t>(ifl), n, st.stream()));
  ZCHK(st.finish());
  if (!retry) for (size_t i = 0; i < n; ++i) if (flags[i]) { zkt_internal_set_error_index(i); return ZKT_ERR_SHAPE; }
  return ZKT_OK;
}

}  // namespace

extern "C" {

// ---- SHA-256 and secp256k1 ECDSA ---------------------------------------------------------------------------------------------------------------------
int zkt_sha256_batch(const uint8_t* msgs, const uint64_t* offsets, size_t n, uint8_t* digests) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!offsets || !digests || (offsets[n] && !msgs)) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; int im, io;
  ZCHK(st.msgs(msgs, offsets, n, im, io));
  const int id = st.out(digests, n * 32);
  ZCHK(st.commit());
  HIPCHK(launch_sha256(st.ptr<uint8_t>(im), st.ptr<unsigned long long>(io), n, st.ptr<uint8_t>(id), st.stream()));
  return st.finish();
}
int zkt_ecdsa_public_keys_batch(const uint64_t* sks, size_t n, zkt_secp_affine* pks) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!sks || !pks) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st;
  const int ik = st.in(sks, n * FRB), ip = st.out(pks, n * SPB);
  ZCHK(st.commit());
  HIPCHK(hipMemcpyAsync(st.small(), &SECP_GEN, SPB, hipMemcpyHostToDevice, st.stream()));
  HIPCHK(launch_generator_mul(G_SECP, st.small(), st.ptr<uint32_t>(ik), st.ptr<uint32_t>(ip), n, st.stream()));      // any 256-bit sk: (sk mod n) G and sk G are the same group element
  return st.finish();
}
int zkt_ecdsa_sign_digest_batch(const uint8_t* digests, const uint64_t* sks, const uint64_t* ks, size_t n, zkt_ecdsa_sig* sigs, uint32_t* retry) {
  if (!digests) return zkt_internal_ready() != ZKT_OK ? ZKT_ERR_DEVICE : ZKT_ERR_SHAPE;
  return ecdsa_sign_host(digests, nullptr, nullptr, sks, ks, n, sigs, retry);
}
int zkt_ecdsa_sign_batch(const uint8_t* msgs, const uint64_t* offsets, const uint64_t* sks, const uint64_t* ks, size_t n, zkt_ecdsa_sig* sigs, uint32_t* retry) {
  return ecdsa_sign_host(nullptr, msgs, offsets, sks, ks, n, sigs, retry);
}
int zkt_ecdsa_verify_digest_batch(const uint8_t* digests, const zkt_ecdsa_sig* sigs, const zkt_secp_affine* pks, size_t n, uint32_t* ok) {
  if (!digests) return zkt_internal_ready() != ZKT_OK ? ZKT_ERR_DEVICE : ZKT_ERR_SHAPE;
  return ecdsa_verify_host(digests, nullptr, nullptr, sigs, pks, n, ok);
}
int zkt_ecdsa_verify_batch(const uint8_t* msgs, const uint64_t* offsets, const zkt_ecdsa_sig* sigs, const zkt_secp_affine* pks, size_t n, uint32_t* ok) {
  return ecdsa_verify_host(nullptr, msgs, offsets, sigs, pks, n, ok);
}
// device pointers, ordered on the caller's stream: nothing is staged and nothing waits (the first call of a process builds the generator's table on that stream and waits for it)
int zkt_ecdsa_verify_digest_batch_dev(const uint8_t* dev_digests, const zkt_ecdsa_sig* dev_sigs, const zkt_secp_affine* dev_pks, size_t n, uint32_t* dev_ok, void* stream) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!dev_digests || !dev_sigs || !dev_pks || !dev_ok) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  const uint32_t* gtab = nullptr;
  { Stage st; ZCHK(secp_generator_table(st, (hipStream_t)stream, &gtab)); }      // for the lock alone: nothing is staged
  HIPCHK(launch_ecdsa_verify(dev_digests, nullptr, nullptr, (const uint32_t*)dev_sigs, (const uint32_t*)dev_pks, gtab, dev_ok, n, (hipStream_t)stream));
  return ZKT_OK;
}

// ---- SHA-512 and Ed25519: bytes in, bytes out --------------------------------------------------------------------------------------------------------
int zkt_sha512_batch(const uint8_t* msgs, const uint64_t* offsets, size_t n, uint8_t* digests) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!offsets || !digests) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; int im, io;
  ZCHK(st.msgs(msgs, offsets, n, im, io));
  const int id = st.out(digests, n * 64);
  ZCHK(st.commit());
  HIPCHK(launch_sha512(st.ptr<uint8_t>(im), st.ptr<unsigned long long>(io), n, st.ptr<uint8_t>(id), st.stream()));
  return st.finish();
}
int zkt_ed25519_decode_batch(const uint8_t* enc, size_t n, uint64_t* xy, uint32_t* on_curve) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!enc || !xy || !on_curve) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st;
  const int ie = st.in(enc, n * 32), ifl = st.out(on_curve, n * 4), ixy = st.out(xy, n * 64);
  ZCHK(st.commit());
  HIPCHK(launch_ed25519_decode(st.ptr<uint8_t>(ie), n, st.ptr<uint32_t>(ixy), st.ptr<uint32_t>(ifl), st.stream()));
  return st.finish();
}
int zkt_ed25519_public_keys_batch(const uint8_t* prv, size_t n, uint8_t* pub) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!prv || !pub) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; const uint32_t* btab = nullptr;
  HIPCHK(ed25519_base_table(&btab, st.stream()));
  const int ik = st.in(prv, n * 32), ip = st.out(pub, n * 32);
  ZCHK(st.commit());
  HIPCHK(launch_ed25519_public_keys(st.ptr<uint8_t>(ik), btab, n, st.ptr<uint8_t>(ip), st.stream()));
  return st.finish();
}
int zkt_ed25519_sign_batch(const uint8_t* msgs, const uint64_t* offsets, const uint8_t* prv, size_t n, uint8_t* sigs) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!offsets || !prv || !sigs) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; const uint32_t* btab = nullptr; int im, io;
  HIPCHK(ed25519_base_table(&btab, st.stream()));
  ZCHK(st.msgs(msgs, offsets, n, im, io));
  const int ik = st.in(prv, n * 32), is = st.out(sigs, n * 64);
  ZCHK(st.commit());
  HIPCHK(launch_ed25519_sign(st.ptr<uint8_t>(im), st.ptr<unsigned long long>(io), st.ptr<uint8_t>(ik), btab, n, st.ptr<uint8_t>(is), st.stream()));
  return st.finish();
}
int zkt_ed25519_verify_batch(const uint8_t* msgs, const uint64_t* offsets, const uint8_t* sigs, const uint8_t* pub, size_t n, uint32_t* ok) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!offsets || !sigs || !pub || !ok) return ZKT_ERR_SHAPE;
  if (n == 0) return ZKT_OK;
  Stage st; const uint32_t* btab = nullptr; int im, io;
  HIPCHK(ed25519_base_table(&btab, st.stream()));
  ZCHK(st.msgs(msgs, offsets, n, im, io));
  const int is = st.in(sigs, n * 64), ip = st.in(pub, n * 32), iok = st.out(ok, n * 4);
  ZCHK(st.commit());
  HIPCHK(launch_ed25519_verify(st.ptr<uint8_t>(im), st.ptr<unsigned long long>(io), st.ptr<uint8_t>(is), st.ptr<uint8_t>(ip), btab, n, st.ptr<uint32_t>(iok), st.stream()));
  return st.finish();
}
// device pointers, ordered on the caller's stream: nothing is staged and nothing waits (but for the first call of a process, which builds the table of B on that stream)
int zkt_ed25519_verify_batch_dev(const uint8_t* dev_msgs, const uint64_t* dev_offsets, const uint8_t* dev_sigs, const uint8_t* dev_pub, size_t n, uint32_t* dev_ok, void* stream) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!dev_offsets || !dev_sigs || !dev_pub || !dev_ok) return ZKT_ERR_SHAPE;      // dev_msgs may be NULL when every message is empty: the offsets are on the device, not looked at here
  if (n == 0) return ZKT_OK;
  const uint32_t* btab = nullptr;
  HIPCHK(ed25519_base_table(&btab, (hipStream_t)stream));
  HIPCHK(launch_ed25519_verify(dev_msgs, (const unsigned long long*)dev_offsets, dev_sigs, dev_pub, btab, n, dev_ok, (hipStream_t)stream));
  return ZKT_OK;
}

}  // extern "C"
