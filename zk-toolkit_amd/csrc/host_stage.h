// The device buffers of ONE host-pointer call of the C ABI (zkt_api.cpp, zkt_hashsig.cpp): a call declares each buffer once, with one size, as an input, an output
// or scratch; commit() reserves the staging arena for exactly that list, carves it and queues the uploads; finish() queues the downloads and waits.
// The layout arithmetic (stage_layout) is pure host code, which the host check exports too (tests/test_stage_layout.py).
// Host code only: no .hip file and no other header includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include "../../include/zkt.h"

namespace zkt {

// the widest call, ECDSA signing: digests or messages + offsets, keys, nonces, signatures, flags
constexpr int STAGE_SLOTS = 6;

// offsets[i] = where slot i of bytes[i] bytes starts, 256-byte aligned, slots in order; returns the bytes the `count` slots take together
inline size_t stage_layout(const size_t* bytes, int count, size_t* offsets) {
  assert(count >= 0 && count <= STAGE_SLOTS);
  size_t total = 0;
  for (int i = 0; i < count; ++i) { offsets[i] = total; total += (bytes[i] + 255) & ~size_t(255); }
  return total;
}

// bytes of the concatenated messages that the n elements can touch.  As in the BLS calls an element whose end lies before its start is an empty message
// (the kernels read no byte of it); unlike there, the upload covers the largest offset, so no element reads past it.
inline size_t msgs_extent(const uint64_t* offsets, size_t n) {
  uint64_t m = 0;
  for (size_t i = 0; i <= n; ++i) m = offsets[i] > m ? offsets[i] : m;
  return (size_t)m;
}

// Holds the library's lock from construction to destruction and runs everything on its staging stream (the caller has set the device: zkt_internal_ready).
// in / out / scratch / inout return the slot's index; a slot of zero bytes is legal and costs no copy.  A device pointer exists only after commit(), which may
// move the arena.  The constructor, commit and the two ends of a call are in zkt_api.cpp, where the arena lives.
class Stage {
 public:
  static constexpr int NONE = -1;                     // ptr(NONE) is null: a buffer this call does not have
  Stage();
  Stage(const Stage&) = delete;
  Stage& operator=(const Stage&) = delete;
  hipStream_t stream() const { return stream_; }
  uint32_t* small() const { return small_; }          // the library's 4 KB of device scratch for one-point values, the lock's holder's to use

  int in(const void* src, size_t bytes) { return add(bytes, src, nullptr, 0); }
  int out(void* dst, size_t bytes) { return add(bytes, nullptr, dst, bytes); }
  int scratch(size_t bytes) { return add(bytes, nullptr, nullptr, 0); }
  // worked on in place: `bytes` go up, the first dst_bytes come down
  int inout(const void* src, size_t bytes, void* dst, size_t dst_bytes) { return add(bytes, src, dst, dst_bytes); }
  // n messages as one byte string with n + 1 offsets: uploads the extent the offsets name, not offsets[n] (a non-monotone vector can end at 0 and still name bytes)
  int msgs(const uint8_t* m, const uint64_t* offsets, size_t n, int& i_msgs, int& i_off) {
    const size_t extent = msgs_extent(offsets, n);
    if (extent && !m) return ZKT_ERR_SHAPE;
    i_msgs = in(m, extent); i_off = in(offsets, (n + 1) * 8);
    return ZKT_OK;
  }

  int commit();                                       // reserve, carve, queue the uploads in the order of declaration
  template <class T> T* ptr(int slot) const {
    assert(base_ && slot < n_);
    return slot < 0 ? nullptr : (T*)(base_ + off_[slot]);
  }
  int finish();                                       // queue the downloads in the order of declaration, wait for the stream
  int finish_err(int code_if_set);                    // the same, then `code_if_set` (and zkt_last_error_index) if a kernel recorded an element in the error word

 private:
  int add(size_t bytes, const void* src, void* dst, size_t dst_bytes) {
    assert(n_ < STAGE_SLOTS && !base_ && dst_bytes <= bytes);
    bytes_[n_] = bytes; src_[n_] = src; dst_[n_] = dst; dst_bytes_[n_] = dst_bytes;
    return n_++;
  }
  int downloads();
  std::unique_lock<std::mutex> lock_;
  hipStream_t stream_;
  uint32_t* small_;
  uint8_t* base_ = nullptr;
  int n_ = 0;
  size_t bytes_[STAGE_SLOTS], off_[STAGE_SLOTS], dst_bytes_[STAGE_SLOTS];
  const void* src_[STAGE_SLOTS];
  void* dst_[STAGE_SLOTS];
};

}  // namespace zkt
