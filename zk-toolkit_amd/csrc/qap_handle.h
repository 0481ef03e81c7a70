// The device-resident QAP of include/zkt.h (zkt_qap_create): three cols x n arrays of canonical Fr coefficients, low degree first — the layout
// zkt_groth16_setup, zkt_qap_quotient and zkt_groth16_prove_qap take from the host, so their kernels read a handle's arrays unchanged.
// Built by zkt_qap.hip; read by the _resident entry points of zkt_poly.hip and zkt_groth16.hip.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

struct zkt_qap {
  size_t n = 0, cols = 0;
  uint32_t* m[3] = {nullptr, nullptr, nullptr};      // ui, vi, wi
  ~zkt_qap() { for (uint32_t* p : m) if (p) (void)hipFree(p); }
  zkt_qap() = default;
  zkt_qap(const zkt_qap&) = delete; zkt_qap& operator=(const zkt_qap&) = delete;
};
