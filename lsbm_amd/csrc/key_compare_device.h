// key_compare_device.h -- the bytewise key compare the device kernels share
// (merge_kernels.hip, memtable_kernels.hip): BytewiseComparator::Compare
// (util/comparator.cc:25-27) over global memory, 8 bytes a step.  Device code
// only; include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

namespace lsbm {
namespace {

typedef const __attribute__((address_space(1))) uint8_t* gcu8;
typedef __attribute__((address_space(1))) uint8_t* gu8;

__device__ __forceinline__ gcu8 gptr(const uint8_t* p, uint64_t off) {
  return reinterpret_cast<gcu8>(reinterpret_cast<uint64_t>(p) + off);
}

__device__ __forceinline__ uint64_t load8(gcu8 p) {
  uint64_t x;
  __builtin_memcpy(&x, p, 8);
  return x;
}

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

}  // namespace
}  // namespace lsbm
