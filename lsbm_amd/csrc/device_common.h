// device_common.h -- the small device helpers the engines' kernels share
// (block, block_build, merge, table_pack, memtable, get, iter): address-space
// and vector typedefs, 8-byte loads and stores at any alignment, the wave
// barrier, wave and workgroup sums, GetVarint32Ptr.  A new engine includes
// this header (key_compare_device.h for key order) instead of copying them.
// Device code only; include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

namespace lsbm {
namespace {

typedef const __attribute__((address_space(1))) uint8_t* gcu8;  // global loads and stores, not flat
typedef __attribute__((address_space(1))) uint8_t* gu8;
typedef __attribute__((address_space(3))) uint8_t* lu8;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* gcu32x4;
typedef __attribute__((address_space(1))) u32x4* gu32x4;

__device__ __forceinline__ gcu8 gptr(const uint8_t* p, uint64_t off) {
  return reinterpret_cast<gcu8>(reinterpret_cast<uint64_t>(p) + off);
}
__device__ __forceinline__ gu8 gwptr(uint8_t* p, uint64_t off) {
  return reinterpret_cast<gu8>(reinterpret_cast<uint64_t>(p) + off);
}

__device__ __forceinline__ uint64_t load8(gcu8 p) {
  uint64_t x;
  __builtin_memcpy(&x, p, 8);
  return x;
}
__device__ __forceinline__ void store8(gu8 p, uint64_t x) { __builtin_memcpy(p, &x, 8); }

// the wave's LDS writes before this point are visible to its reads after it
__device__ __forceinline__ void wave_phase() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// one lane per item in workgroups of kThreads lanes: this lane's item
template <uint32_t kThreads>
__device__ __forceinline__ uint64_t global_index() {
  return (uint64_t)blockIdx.x * kThreads + threadIdx.x;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, uint32_t lane) {
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive sum of v over the lanes of a workgroup of kWaves waves, in lane
// order, and the total; lds: kWaves words, free again on return
template <uint32_t kWaves>
__device__ __forceinline__ void block_excl_sum(uint64_t v, uint64_t* lds, uint64_t& excl, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan(v, lane);
  if (lane == 63) lds[w] = incl;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
  for (uint32_t i = 0; i < kWaves; i++) {
    const uint64_t t = lds[i];
    if (i < w) before += t;
    total += t;
  }
  __syncthreads();  // (the row is free for the caller's next round)
  excl = before + incl - v;
}

// GetVarint32Ptr (util/coding.cc:112-129) over d[p, limit): at most 5 bytes,
// never past limit; the fifth byte's bits above 2^32 are dropped as the
// reference's shift does.  P: any byte pointer; I: the position's type.
template <class P, class I>
__device__ __forceinline__ bool varint32(P d, I& p, I limit, uint32_t& v) {
  uint32_t r = 0;
  for (uint32_t shift = 0; shift <= 28 && p < limit; shift += 7) {
    const uint32_t byte = d[p++];
    if (byte & 128u) {
      r |= (byte & 127u) << shift;
    } else {
      v = r | (byte << shift);
      return true;
    }
  }
  return false;
}

}  // namespace
}  // namespace lsbm
