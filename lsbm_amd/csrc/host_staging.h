// host_staging.h -- typed staging for the C++ host layers that work through a
// HostSession's scratch slots (block_reader.cc, block_builder.cc,
// compaction.cc, memtable_flush.cc, filter_block.cc, block_compression.cc).
// Packed describes a buffer that holds several arrays back to back, once, for
// the device pointers and the host's read-back alike; Staging is one call's
// session with typed scratch requests and copies and one sticky error.
// LSBM_STAGING_LAYOUT_ONLY leaves out everything but Packed (no HIP headers).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#ifndef LSBM_STAGING_LAYOUT_ONLY
#include <type_traits>
#include <vector>

#include "host_session.h"
#endif

#pragma GCC visibility push(hidden)  // (the layers' objects export by default)
namespace lsbm {

// `count` elements of T at byte `offset` of a packed buffer.
template <class T>
struct Field {
  size_t offset, count;
  size_t bytes() const { return count * sizeof(T); }
  // The field in the buffer at `base` (nullptr stays nullptr: a failed Staging::buf).
  T* in(void* base) const { return base ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + offset) : nullptr; }
  const T* in(const void* base) const { return in(const_cast<void*>(base)); }
};

// Fields lie back to back in the order they are added, with no padding:
// declare the widest element type first (u64, then u32, then u8).
class Packed {
 public:
  template <class T>
  Field<T> add(size_t count) {
    assert(bytes_ % sizeof(T) == 0);  // a narrower field was added before a wider one
    const Field<T> f{bytes_, count};
    bytes_ += f.bytes();
    return f;
  }
  size_t bytes() const { return bytes_; }

 private:
  size_t bytes_ = 0;
};

#ifndef LSBM_STAGING_LAYOUT_ONLY
// The first HIP error sticks: every later buf / put / get does nothing (buf
// returns nullptr), and a layer tests ok() before each launch.
class Staging {
 public:
  Status Open(int device) { return ss_.Open(device); }
  hipStream_t stream() { return ss_->stream(); }
  // Device scratch slot `slot`, at least `count` elements of T and never empty:
  // the pointer is never null and never what an earlier call left in the slot
  // (the entry points reject a null pointer whatever the size).
  template <class T>
  T* buf(int slot, size_t count) {
    void* p = nullptr;
    if (ok()) e_ = ss_->scratch(slot, count ? count * sizeof(T) : 1, &p);
    return ok() ? static_cast<T*>(p) : nullptr;
  }
  // Host -> device / device -> host of `count` elements (bytes are char on one side, uint8_t on the other).
  template <class T, class U>
  void put(T* d, const U* h, size_t count) {
    static_assert(std::is_integral<U>::value && sizeof(T) == sizeof(U), "element types differ");
    if (ok()) e_ = ss_->upload(d, h, count * sizeof(T));
  }
  template <class T, class U>
  void get(T* h, const U* d, size_t count) {
    static_assert(std::is_integral<U>::value && sizeof(T) == sizeof(U), "element types differ");
    if (ok()) e_ = ss_->download(h, d, count * sizeof(T));
  }
  void put_pieces(uint8_t* d, const std::vector<HostSession::Piece>& pieces) {
    if (ok()) e_ = ss_->upload_pieces(d, pieces.data(), pieces.size());
  }
  // The result of a HIP call the layer makes itself.
  void note(hipError_t e) { e_ = ok() ? e : e_; }
  bool ok() const { return e_ == hipSuccess; }
  Status status(const char* what) const { return hip_status(e_, what); }

 private:
  SessionLease ss_;
  hipError_t e_ = hipSuccess;
};

inline Status check_offsets(const uint64_t* offsets, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return Status::InvalidArgument("offsets must not decrease");
  return Status::OK();
}

// Rebase offsets[0..n] to start at 0 (the staged copy starts at offsets[0]).
inline std::vector<uint64_t> rebased(const uint64_t* offsets, size_t n) {
  std::vector<uint64_t> r(n + 1);
  for (size_t i = 0; i <= n; i++) r[i] = offsets[i] - offsets[0];
  return r;
}
#endif  // LSBM_STAGING_LAYOUT_ONLY

}  // namespace lsbm
#pragma GCC visibility pop
