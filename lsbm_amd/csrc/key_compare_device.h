// key_compare_device.h -- the key order the device kernels share (merge,
// memtable, get, iter): BytewiseComparator::Compare (util/comparator.cc:25-27)
// over global memory, 8 bytes a step, and InternalKeyComparator::Compare
// (common/dbformat.cc) on top of it.  Device code only; include after
// <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

#include "device_common.h"  // gcu8, gptr, load8

namespace lsbm {
namespace {

// memcmp over the shorter length, then the lengths: < 0, 0, > 0
__device__ __forceinline__ int bytes_compare(gcu8 a, uint64_t alen, gcu8 b, uint64_t blen) {
  const uint64_t m = alen < blen ? alen : blen;
  uint64_t i = 0;
  while (i + 8 <= m) {
    const uint64_t x = load8(a + i), y = load8(b + i);
    if (x != y) {
      // the first byte that differs in memory is the lowest differing byte of
      // the little-endian word: compare that byte, not the words
      const uint32_t sh = (uint32_t)__builtin_ctzll(x ^ y) & ~7u;
      return ((x >> sh) & 0xff) < ((y >> sh) & 0xff) ? -1 : 1;
    }
    i += 8;
  }
  if (i < m && m >= 8) {
    // the tail as one more word that ends at m: the bytes it repeats are equal,
    // so its first difference is the tail's (not up to 7 dependent byte loads)
    const uint64_t x = load8(a + (m - 8)), y = load8(b + (m - 8));
    if (x != y) {
      const uint32_t sh = (uint32_t)__builtin_ctzll(x ^ y) & ~7u;
      return ((x >> sh) & 0xff) < ((y >> sh) & 0xff) ? -1 : 1;
    }
    i = m;
  }
  while (i < m) {
    const uint8_t p = a[i], q = b[i];
    if (p != q) return p < q ? -1 : 1;
    i++;
  }
  return alen < blen ? -1 : (alen > blen ? 1 : 0);
}

// the tie-break of two internal keys whose user keys are equal, on their
// 8-byte tags (sequence << 8 | type): the larger tag sorts first
__device__ __forceinline__ int tag_compare(uint64_t a, uint64_t b) { return a > b ? -1 : (a < b ? 1 : 0); }

// InternalKeyComparator::Compare of a stored key (at `at`, `len` >= 8 bytes of
// `buf`) with the lookup key (user key u of ulen bytes, tag), which may exist
// only in registers: < 0, 0, > 0
__device__ __forceinline__ int internal_compare(const uint8_t* buf, uint64_t at, uint64_t len, gcu8 u, uint64_t ulen,
                                                uint64_t tag) {
  const int c = bytes_compare(gptr(buf, at), len - 8, u, ulen);
  if (c) return c;
  return tag_compare(load8(gptr(buf, at + len - 8)), tag);
}

}  // namespace
}  // namespace lsbm
