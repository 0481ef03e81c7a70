// What the Groth16 verifier keeps per verifying key, for the last few keys seen (zkt_groth16_vk_cache.cpp): fixed-base tables of the statement points, and the
// key's entry for the 63-step verification kernel.  Host code only; read by zkt_groth16.hip.  zkt_shutdown releases both (groth16_vk_clear_caches, zkt_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include "../../include/zkt.h"

namespace zkt {
// Device tables for the n_stmt points at host pointer `pts` (device copy dU), or null when they could not be provided (the caller falls back).
// The caller keeps the returned reference until its launches have completed: an entry evicted meanwhile is released only when its last user lets go.
std::shared_ptr<void> stmt_tables_for(const zkt_g1_affine* pts, size_t n_stmt, const uint32_t* dU, hipStream_t s);

enum { ATE_READY = 0, ATE_UNUSABLE, ATE_ABSENT, ATE_BUSY };
// READY: *out holds the entry (keep the reference until the launches that read it have completed).  UNUSABLE: the key keeps the value-comparing kernels.  ABSENT: never seen
// (AteBuild::begin).  BUSY: another call is building it right now.
int ate_key_lookup(const zkt_groth16_crs* c, size_t n_stmt, std::shared_ptr<void>* out);
// Builds the entry of a key that ate_key_lookup reported ABSENT, beside the call that brought it: begin ... tables, or abandon when the scope is left early.
struct AteBuild {
  int idx = -1; hipStream_t s = nullptr;      // idx stays -1 when begin started nothing: the caller carries on without
  void begin(const zkt_groth16_crs* c, size_t n_stmt, const uint32_t* dU, const uint32_t* dg, const uint32_t* dd, hipStream_t s);      // `s` (the call's stream) holds dU, dg, dd
  void tables(const uint32_t* tab16);                                                                                              // once `s` holds the statement points' 16^k tables
  ~AteBuild();
};
// the entry, built now if need be and waited for (large batches, zkt_groth16_vk_prepare); null: the value-comparing kernels
std::shared_ptr<void> ate_key_now(const zkt_groth16_crs* c, size_t n_stmt, const uint32_t* dU, const uint32_t* dg, const uint32_t* dd, hipStream_t s);
}  // namespace zkt
