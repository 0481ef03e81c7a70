// What the dense-polynomial files (zkt_poly.hip, zkt_qap.hip) share on the host side: the stream-ordered scratch of one call, and the two routines of
// zkt_poly.hip that the QAP build needs as well.  Host code only.
#pragma once
#include <vector>
#include "host_abi.h"

namespace zkt {
// stream-ordered scratch of one call: taken on the call's stream, given back on it when the call's frame ends
struct Pool {
  hipStream_t s; std::vector<void*> ptrs;
  explicit Pool(hipStream_t s_) : s(s_) {}
  uint32_t* get(size_t elems) {
    void* p = nullptr;
    if (hipMallocAsync(&p, (elems ? elems : 1) * FRB, s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ptrs.push_back(p); return (uint32_t*)p;
  }
  ~Pool() { for (void* p : ptrs) (void)hipFreeAsync(p, s); }
  Pool(const Pool&) = delete; Pool& operator=(const Pool&) = delete;
};
#define PGET(var, pool, elems) uint32_t* var = (pool).get(elems); if (!var) return ZKT_ERR_DEVICE

// ---- zkt_poly.hip ----
// out[0 .. n] = the coefficients of prod_{i=1..n} (x - i), Montgomery (queued on the pool's stream)
int build_t_dev(Pool& pool, size_t n, uint32_t* out);
// Montgomery device values -> canonical host words (queued)
int store_host(uint64_t* dst, const uint32_t* src, size_t cnt, Pool& pool);
}  // namespace zkt
