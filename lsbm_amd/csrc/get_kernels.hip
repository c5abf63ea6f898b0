// get_kernels.hip -- gfx950 kernels of the batched DB::Get (include/lsbm_get.h):
// LookupKey (common/dbformat.cc:121-137), MemTable::Get (common/memtable.cc:109-144),
// FindFile with the tests beside it (lsbm/version_set.cc:130-150, :364-374) and
// SaveValue with its switch (lsbm/version_set.cc:227-240, :392-407).
//
// get_offsets_kernel    one lane per key of an offsets array: it does not
//                       decrease, stays inside its buffer and has the bytes
//                       the caller needs; else the status word is set.
// lookup_check_kernel   the same for the user keys, and the output's room.
// lookup_keys_kernel    one lane per query: user key || fixed64(seq << 8 | 1).
// mem_get_kernel        one lane per query: lower bound over the sorted
//                       memtable, then the user-key and type tests.
// run_check_kernel      one lane per run: its file range is inside the files.
// find_file_kernel      one lane per (query, run): FindFile's binary search or
//                       Level 0's range test.
// save_check_kernel     one lane per query: the states are known and every
//                       key the callback will parse is inside its window.
// save_value_kernel     one lane per query: the callback and the switch.
// slices_gather_kernel  kGatherLanes lanes per query: the value bytes.
//
// Every kernel that reads key bytes runs after the check kernels of its call
// on the same stream and leaves at once when they set the status word, so key
// bytes are addressed only through offsets that were checked.  File and entry
// indices come from binary searches over [0, n) and are below n.  Every loop
// halves a range or advances.  No LDS, no spin-waits, no cross-workgroup state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // gcu8, gu8, gptr, gwptr, load8, store8, global_index
#include "get_types.h"
#include "key_compare_device.h"  // bytes_compare, internal_compare

namespace lsbm {
namespace {

__global__ __launch_bounds__(kGetThreads) void get_offsets_kernel(OffsetsArgs a) {
  const uint64_t i = global_index<kGetThreads>();
  if (i >= a.n) return;
  const uint64_t lo = a.offsets[i], hi = a.offsets[i + 1];
  if (lo > hi || hi > a.size || hi - lo < a.min_len) atomicOr(a.status, kGetBadInput);
}

__global__ __launch_bounds__(kGetThreads) void lookup_check_kernel(LookupArgs a) {
  const uint64_t i = global_index<kGetThreads>();
  if (i > a.n) return;
  const uint64_t lo = a.user_offsets[i];
  bool bad = lo > a.user_size;
  if (i < a.n) {
    bad = bad || lo > a.user_offsets[i + 1];
  } else {  // the room: every key before this offset is inside user_size, so the sum cannot wrap
    bad = bad || a.keys_cap < 8 * a.n || a.keys_cap - 8 * a.n < lo;
  }
  if (bad) atomicOr(a.status, kGetBadInput);
}

__global__ __launch_bounds__(kGetThreads) void lookup_keys_kernel(LookupArgs a) {
  const uint64_t q = global_index<kGetThreads>();
  if (q > a.n || *a.status) return;
  const uint64_t lo = a.user_offsets[q];
  a.key_offsets[q] = lo + 8 * q;
  if (q == a.n) return;
  const uint64_t len = a.user_offsets[q + 1] - lo;
  const gcu8 src = gptr(a.user_keys, lo);
  const gu8 dst = gwptr(a.keys, lo + 8 * q);
  uint64_t i = 0;
  for (; i + 8 <= len; i += 8) store8(dst + i, load8(src + i));
  for (; i < len; i++) dst[i] = src[i];
  const uint64_t seq = a.snapshots ? a.snapshots[q] : a.snapshot;
  store8(dst + len, (seq << 8) | 1u);  // kValueTypeForSeek = kTypeValue
}

__global__ __launch_bounds__(kGetThreads) void mem_get_kernel(MemGetArgs a) {
  const uint64_t q = global_index<kGetThreads>();
  if (q >= a.q.n || *a.q.status || a.q.verdict[q] != kGetUndecided) return;
  const uint64_t ka = a.q.key_offsets[q], ulen = a.q.key_offsets[q + 1] - ka - 8;
  const gcu8 u = gptr(a.q.keys, ka);
  const uint64_t tag = load8(u + ulen);
  // Seek: the first entry that is not before the lookup key
  uint64_t lo = 0, hi = a.n_entries;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t ea = a.mem_key_offsets[mid], el = a.mem_key_offsets[mid + 1] - ea;
    if (internal_compare(a.mem_keys, ea, el, u, ulen, tag) < 0) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  if (lo >= a.n_entries) return;
  const uint64_t ea = a.mem_key_offsets[lo], el = a.mem_key_offsets[lo + 1] - ea;
  if (bytes_compare(gptr(a.mem_keys, ea), el - 8, u, ulen) != 0) return;
  const uint32_t type = (uint32_t)(load8(gptr(a.mem_keys, ea + el - 8)) & 0xff);
  if (type == 1) {
    a.q.value[2 * q] = a.mem_values[2 * lo];
    a.q.value[2 * q + 1] = a.mem_values[2 * lo + 1];
    a.q.verdict[q] = kGetFound;
  } else if (type == 0) {
    a.q.value[2 * q] = 0;
    a.q.value[2 * q + 1] = 0;
    a.q.verdict[q] = kGetDeleted;
  } else {
    return;  // (the reference's switch has no other case: the entry is passed over)
  }
  a.q.where[q] = a.q.source_id;
}

__global__ __launch_bounds__(kGetThreads) void run_check_kernel(FindFileArgs a) {
  const uint64_t r = global_index<kGetThreads>();
  if (r >= a.n_runs) return;
  const uint64_t first = a.run_first[r], last = a.run_first[r + 1];
  if (first > last || last > a.n_files || ((a.run_flags[r] & kRunLevel0) && last - first > 1))
    atomicOr(a.status, kGetBadInput);
}

__global__ __launch_bounds__(kGetThreads) void find_file_kernel(FindFileArgs a) {
  const uint64_t idx = global_index<kGetThreads>();
  if (idx >= a.n * a.n_runs) return;
  const uint64_t q = idx / a.n_runs, r = idx - q * a.n_runs;
  int32_t file = -1;
  const uint64_t first = a.run_first[r], last = a.run_first[r + 1];
  const uint32_t flags = a.run_flags[r];
  if (!*a.status && first < last) {  // (bad input: every word is -1)
    const uint64_t ka = a.key_offsets[q], ulen = a.key_offsets[q + 1] - ka - 8;
    const gcu8 u = gptr(a.keys, ka);
    uint64_t f = first;
    bool inside;
    if (flags & kRunLevel0) {
      const uint64_t la = a.bound_offsets[2 * f + 1], ll = a.bound_offsets[2 * f + 2] - la;
      inside = bytes_compare(u, ulen, gptr(a.bounds, la), ll - 8) <= 0;
    } else {
      const uint64_t tag = load8(u + ulen);
      uint64_t left = first, right = last;
      while (left < right) {
        const uint64_t mid = left + (right - left) / 2;
        const uint64_t la = a.bound_offsets[2 * mid + 1], ll = a.bound_offsets[2 * mid + 2] - la;
        if (internal_compare(a.bounds, la, ll, u, ulen, tag) < 0) {
          left = mid + 1;
        } else {
          right = mid;
        }
      }
      f = right;
      inside = f < last && a.visible[f] != 0;
    }
    if (inside) {
      const uint64_t sa = a.bound_offsets[2 * f], sl = a.bound_offsets[2 * f + 1] - sa;
      if (bytes_compare(u, ulen, gptr(a.bounds, sa), sl - 8) >= 0) file = (int32_t)f;
    }
  }
  a.file[idx] = file;
}

__global__ __launch_bounds__(kGetThreads) void save_check_kernel(SaveArgs a) {
  const uint64_t q = global_index<kGetThreads>();
  if (q >= a.q.n) return;
  const uint32_t state = a.state[q];
  bool bad = state > kStateMax;
  if (state == kStateValid && a.q.verdict[q] == kGetUndecided && a.key_len[q] >= 8) {
    const uint64_t lo = a.found_offsets[q], hi = a.found_offsets[q + 1];
    bad = bad || lo > hi || hi > a.found_size || hi - lo < a.key_len[q];
  }
  if (bad) atomicOr(a.q.status, kGetBadInput);
}

__global__ __launch_bounds__(kGetThreads) void save_value_kernel(SaveArgs a) {
  const uint64_t q = global_index<kGetThreads>();
  if (q >= a.q.n || *a.q.status || a.q.verdict[q] != kGetUndecided) return;
  const uint32_t state = a.state[q];
  if (state == kStateNotValid || state == kStateFiltered) return;
  uint32_t verdict;
  uint64_t v0 = 0, v1 = 0;
  if (state != kStateValid) {
    verdict = kGetError + state;  // if (!s.ok()) return s
  } else {
    const uint64_t flen = a.key_len[q];
    verdict = kGetCorrupt;  // ParseInternalKey: n < 8
    if (flen >= 8) {
      const gcu8 f = gptr(a.found, a.found_offsets[q]);
      const uint32_t type = (uint32_t)(load8(f + flen - 8) & 0xff);
      if (type <= 1) {
        const uint64_t ka = a.q.key_offsets[q], ulen = a.q.key_offsets[q + 1] - ka - 8;
        if (bytes_compare(f, flen - 8, gptr(a.q.keys, ka), ulen) != 0) return;  // another user key: kNotFound
        verdict = type == 1 ? kGetFound : kGetDeleted;
        if (type == 1) {
          v0 = a.value_in[2 * q];
          v1 = a.value_in[2 * q + 1];
        }
      }
    }
  }
  a.q.value[2 * q] = v0;
  a.q.value[2 * q + 1] = v1;
  a.q.where[q] = a.q.source_id;
  a.q.verdict[q] = verdict;
}

__global__ __launch_bounds__(kGetThreads) void slices_gather_kernel(GatherArgs a) {
  const uint64_t idx = global_index<kGetThreads>();
  const uint64_t q = idx / kGatherLanes;
  const uint32_t lane = (uint32_t)(idx % kGatherLanes);
  if (q >= a.n) return;
  const int32_t w = a.where[q];
  if (w < a.where_lo || w >= a.where_hi) return;
  const uint64_t at = a.slices[2 * q], len = a.slices[2 * q + 1];
  const uint64_t lo = a.out_offsets[q], hi = a.out_offsets[q + 1];
  if (at > a.image_size || len > a.image_size - at || lo > hi || hi > a.out_cap || len > hi - lo) {
    if (lane == 0) atomicOr(a.status, kGetBadInput);
    return;
  }
  const gcu8 src = gptr(a.image, at);
  const gu8 dst = gwptr(a.out, lo);
  for (uint64_t i = lane; i < len; i += kGatherLanes) dst[i] = src[i];
}

uint32_t groups(uint64_t n) { return (uint32_t)((n + kGetThreads - 1) / kGetThreads); }

void check_offsets(const uint64_t* offsets, uint64_t n, uint64_t size, uint64_t min_len, uint32_t* status,
                   hipStream_t stream) {
  if (!n) return;
  const OffsetsArgs c = {offsets, n, size, min_len, status};
  hipLaunchKernelGGL(get_offsets_kernel, dim3(groups(n)), dim3(kGetThreads), 0, stream, c);
}

}  // namespace

hipError_t launch_lookup_keys(const LookupArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const dim3 grid(groups(a.n + 1)), block(kGetThreads);
  hipLaunchKernelGGL(lookup_check_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(lookup_keys_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_memtable_get(const MemGetArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.q.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  check_offsets(a.mem_key_offsets, a.n_entries, a.mem_keys_size, 8, a.q.status, stream);
  check_offsets(a.q.key_offsets, a.q.n, a.q.keys_size, 8, a.q.status, stream);
  if (a.q.n) hipLaunchKernelGGL(mem_get_kernel, dim3(groups(a.q.n)), dim3(kGetThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_find_file(const FindFileArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  check_offsets(a.bound_offsets, 2 * a.n_files, a.bounds_size, 8, a.status, stream);
  check_offsets(a.key_offsets, a.n, a.keys_size, 8, a.status, stream);
  if (a.n_runs) hipLaunchKernelGGL(run_check_kernel, dim3(groups(a.n_runs)), dim3(kGetThreads), 0, stream, a);
  if (a.n * a.n_runs)
    hipLaunchKernelGGL(find_file_kernel, dim3(groups(a.n * a.n_runs)), dim3(kGetThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_save_value(const SaveArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.q.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  check_offsets(a.q.key_offsets, a.q.n, a.q.keys_size, 8, a.q.status, stream);
  if (a.q.n) {
    const dim3 grid(groups(a.q.n)), block(kGetThreads);
    hipLaunchKernelGGL(save_check_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(save_value_kernel, grid, block, 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_slices_gather(const GatherArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  if (a.n)
    hipLaunchKernelGGL(slices_gather_kernel, dim3(groups(a.n * kGatherLanes)), dim3(kGetThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
