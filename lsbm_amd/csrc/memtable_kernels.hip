// memtable_kernels.hip -- gfx950 kernels of the memtable flush
// (include/lsbm_memtable.h): WriteBatch::Iterate (common/write_batch.cc:42-80)
// over many log records, MemTable::Add's internal keys (common/memtable.cc:83-107)
// and the skiplist's order (common/skiplist.h:334-367) as a sort.
//
// wb_scan_kernel       one lane per record: the walk; entries, user-key bytes
//                      and the status.
// wb_decode_kernel     one lane per record: the same walk written out -- the
//                      internal keys, their offsets, the value slices -- and
//                      the largest sequence number.
// mem_check_kernel     one lane per entry: its key's offsets and length, and
//                      how many bytes its user key shares with entry 0's; the
//                      least of these is the prefix every user key starts with.
// mem_tile_sort_kernel one workgroup per tile of kMemThreads entries: each
//                      lane makes its entry's sort word (the 7 user-key bytes
//                      after that prefix big-endian, then min(bytes left, 8)) and the
//                      tile is sorted in LDS as {word, entry} pairs by a
//                      bitonic network; only equal words go to the keys.
// mem_merge_kernel     one lane per position of a pass: the entry counts the
//                      entries of its sibling run that come before it (a binary
//                      search; the order is total, so no tie rule) and stores
//                      its pair at its rank in the other ping-pong set.
// mem_len_kernel       per tile of sorted positions the key bytes.
// mem_scan_kernel      one workgroup: running sums over the tiles, the counts
//                      and the status.
// mem_emit_kernel      one lane per sorted position: source and out_key_offsets.
//
// The walks read only inside their record, which is checked against the image
// first, and write only inside their record's windows.  Every sort kernel
// after mem_check runs only when no entry is in error, that is on key offsets
// that were checked; an entry index read back from scratch is checked against
// n before it addresses anything.  Every loop halves a range or advances.  No
// spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"       // gcu8, gu8, gptr, gwptr, load8, store8, varint32, wave_incl_scan
#include "key_compare_device.h"  // bytes_compare
#include "memtable_types.h"

namespace lsbm {
namespace {

constexpr uint32_t kTypeValue = 1;                     // common/dbformat.h (kTypeDeletion is 0)
constexpr uint32_t kWbHeader = 12;                     // common/write_batch.cc:26
constexpr uint32_t kNoEntry = 0xffffffffu;             // the padding of the last tile: word ~0, sorts last
constexpr uint32_t kMergeBadInput = 2;                 // LSBM_MERGE_BAD_INPUT

// GetLengthPrefixedSlice: the slice is image[at, at + len) and pos moves past it
__device__ __forceinline__ bool get_slice(gcu8 img, uint64_t& pos, uint64_t end, uint64_t& at, uint32_t& len) {
  if (!varint32(img, pos, end, len) || len > end - pos) return false;
  at = pos;
  pos += len;
  return true;
}

template <bool kWrite>
__device__ __forceinline__ void wb_walk(const WbArgs& a, uint64_t r) {
  const uint64_t off = a.records[2 * r], len = a.records[2 * r + 1];
  uint32_t st = kWbOk;
  uint64_t found = 0, user_bytes = 0;
  if (off > a.image_size || len > a.image_size - off || len > 0xffffffffull) {
    st = kWbBadInput;
  } else if (len < kWbHeader) {
    st = kWbTooSmall;
  } else {
    const gcu8 img = gptr(a.image, 0);
    const uint64_t seq = load8(img + off);
    const uint32_t count = (uint32_t)img[off + 8] | (uint32_t)img[off + 9] << 8 | (uint32_t)img[off + 10] << 16 |
                           (uint32_t)img[off + 11] << 24;
    uint64_t e = 0, e_end = 0, k = 0, k_end = 0;
    if (kWrite) {
      // Sequence + Count - 1 with Count an int (lsbm/db_impl.cc:456-458)
      atomicMax(reinterpret_cast<unsigned long long*>(a.max_sequence),
                (unsigned long long)(seq + (uint64_t)(int64_t)(int32_t)count - 1));
      e = a.entry_base[r];
      e_end = a.entry_base[r + 1];
      k = a.key_base[r];
      k_end = a.key_base[r + 1];
      if (e > e_end || e_end > a.entries_cap || k > k_end || k_end > a.keys_cap) st = kWbNoRoom;
    }
    const uint64_t end = off + len;
    uint64_t pos = off + kWbHeader;
    while (st == kWbOk && pos < end) {
      const uint32_t tag = img[pos++];
      if (tag > kTypeValue) {
        st = kWbUnknownTag;
        break;
      }
      uint64_t key_at = 0, value_at = 0;
      uint32_t key_len = 0, value_len = 0;
      if (!get_slice(img, pos, end, key_at, key_len)) {
        st = tag == kTypeValue ? kWbBadPut : kWbBadDelete;
        break;
      }
      value_at = pos;
      if (tag == kTypeValue && !get_slice(img, pos, end, value_at, value_len)) {
        st = kWbBadPut;
        break;
      }
      if (kWrite) {
        if (e >= e_end || (uint64_t)key_len + 8 > k_end - k) {
          st = kWbNoRoom;
          break;
        }
        const gu8 dst = gwptr(a.keys, k);
        uint32_t i = 0;
        for (; i + 8 <= key_len; i += 8) {
          store8(dst + i, load8(img + key_at + i));
        }
        for (; i < key_len; i++) dst[i] = img[key_at + i];
        const uint64_t packed = (seq + found) << 8 | tag;  // MemTable::Add
        store8(dst + key_len, packed);
        a.key_offsets[e] = k;
        a.values[2 * e] = value_at;
        a.values[2 * e + 1] = value_len;
        e++;
        k += (uint64_t)key_len + 8;
      }
      found++;  // the handler was called
      user_bytes += key_len;
    }
    if (st == kWbOk && (uint32_t)found != count) st = kWbWrongCount;
  }
  if (!kWrite) {
    a.counts[2 * r] = found;
    a.counts[2 * r + 1] = user_bytes;
  }
  a.status[r] = st;
}

__global__ __launch_bounds__(kMemThreads) void wb_scan_kernel(WbArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kMemThreads + threadIdx.x;
  if (r < a.n_records) wb_walk<false>(a, r);
}

__global__ __launch_bounds__(kMemThreads) void wb_decode_kernel(WbArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kMemThreads + threadIdx.x;
  if (r < a.n_records) wb_walk<true>(a, r);
  if (r == 0) {
    // the slot after the last entry (the windows are running sums: every other
    // slot is the first entry of a record that follows)
    const uint64_t e = a.entry_base[a.n_records];
    if (e <= a.entries_cap) a.key_offsets[e] = a.key_base[a.n_records];
  }
}

// ---------------------------------------------------------------- sort

// bytes the user keys at [ka, ka + ua) and [kb, kb + ub) have in common at their start
__device__ __forceinline__ uint64_t common_prefix(const MemSortArgs& a, uint64_t ka, uint64_t ua, uint64_t kb, uint64_t ub) {
  const uint64_t m = ua < ub ? ua : ub;
  const gcu8 x = gptr(a.keys, ka), y = gptr(a.keys, kb);
  uint64_t i = 0;
  for (; i + 8 <= m; i += 8) {
    const uint64_t d = load8(x + i) ^ load8(y + i);
    if (d) return i + ((uint32_t)__builtin_ctzll(d) >> 3);
  }
  while (i < m && x[i] == y[i]) i++;
  return i;
}

__global__ __launch_bounds__(kMemThreads) void mem_check_kernel(MemSortArgs a) {
  const uint32_t e = blockIdx.x * kMemThreads + threadIdx.x;
  uint32_t shared = 0xffffffffu;  // with key 0's user key
  if (e < a.n) {
    const uint64_t ka = a.key_offsets[e], kb = a.key_offsets[e + 1];
    if (ka > kb || kb > a.keys_size || kb - ka < 8) {
      atomicOr(a.err, 1u);
    } else {
      const uint64_t za = a.key_offsets[0], zb = a.key_offsets[1];
      if (za <= zb && zb <= a.keys_size && zb - za >= 8) {  // (else entry 0's own lane reports it)
        const uint64_t c = common_prefix(a, ka, kb - ka - 8, za, zb - za - 8);
        shared = c < 0xffffffffu ? (uint32_t)c : 0xfffffffeu;
      }
    }
  }
  for (uint32_t o = 32; o > 0; o >>= 1) {
    const uint32_t other = __shfl_xor(shared, o);
    shared = other < shared ? other : shared;
  }
  if ((threadIdx.x & 63) == 0 && shared != 0xffffffffu) atomicMin(a.skip, shared);
}

// the sort word of the key at [ka, ka + klen), klen >= 8, when every user key
// starts with the same `skip` bytes: the 7 user-key bytes after them
// big-endian, zero-padded, then min(user-key bytes after them, 8).  Words that
// differ order their keys; equal words below 8 in the low byte are equal user
// keys, and with 8 there the user keys agree in skip + 7 bytes and their rest
// is compared.
__device__ __forceinline__ uint64_t sort_word(const MemSortArgs& a, uint64_t ka, uint64_t klen, uint64_t skip) {
  const uint64_t ulen = klen - 8, at = skip < ulen ? skip : ulen, rest = ulen - at;
  const uint64_t be = __builtin_bswap64(load8(gptr(a.keys, ka + at)));  // (8 bytes of the key: klen - at >= 8)
  const uint32_t take = rest < 7 ? (uint32_t)rest : 7;
  const uint64_t mask = take ? ~0ull << (64 - 8 * take) : 0;
  return (be & mask) | (rest < 8 ? rest : 8);
}

// entry ia (word wa) comes before entry ib (word wb) in the memtable's order:
// user key ascending, tag descending, later arrival first
__device__ __forceinline__ bool entry_less(const MemSortArgs& a, uint64_t skip, uint64_t wa, uint32_t ia, uint64_t wb,
                                           uint32_t ib) {
  if (wa != wb) return wa < wb;
  if (ia == ib || ia >= a.n || ib >= a.n) return false;  // (padding, or scratch that is not trusted)
  const uint64_t ka = a.key_offsets[ia], la = a.key_offsets[ia + 1] - ka;
  const uint64_t kb = a.key_offsets[ib], lb = a.key_offsets[ib + 1] - kb;
  const uint64_t done = skip + 7;  // user-key bytes the equal words stand for
  if ((wa & 0xff) == 8 && la >= done + 9 && lb >= done + 9) {  // (8 there: a user key of skip + 8 bytes or more)
    const int c = bytes_compare(gptr(a.keys, ka + done), la - 8 - done, gptr(a.keys, kb + done), lb - 8 - done);
    if (c) return c < 0;
  }
  const uint64_t ta = load8(gptr(a.keys, ka + la - 8)), tb = load8(gptr(a.keys, kb + lb - 8));
  if (ta != tb) return ta > tb;  // (key_compare_device.h's tag_compare, spelled out: it compiles differently here)
  return ia > ib;
}

__global__ __launch_bounds__(kMemThreads) void mem_tile_sort_kernel(MemSortArgs a) {
  __shared__ uint64_t s_w[kMemThreads];
  __shared__ uint32_t s_i[kMemThreads];
  if (*a.err) return;  // (uniform)
  const uint32_t t = threadIdx.x, p = blockIdx.x * kMemThreads + t;
  const uint64_t skip = *a.skip;
  uint64_t w = ~0ull;
  uint32_t idx = kNoEntry;
  if (p < a.n) {
    const uint64_t ka = a.key_offsets[p];
    w = sort_word(a, ka, a.key_offsets[p + 1] - ka, skip);
    idx = p;
  }
  s_w[t] = w;
  s_i[t] = idx;
  for (uint32_t k = 2; k <= (uint32_t)kMemThreads; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const uint32_t q = t ^ j;
      if (q > t) {
        const uint64_t w0 = s_w[t], w1 = s_w[q];
        const uint32_t i0 = s_i[t], i1 = s_i[q];
        const bool up = (t & k) == 0;
        if (up ? entry_less(a, skip, w1, i1, w0, i0) : entry_less(a, skip, w0, i0, w1, i1)) {
          s_w[t] = w1;
          s_i[t] = i1;
          s_w[q] = w0;
          s_i[q] = i0;
        }
      }
    }
  }
  __syncthreads();
  if (p < a.n) {
    a.word[0][p] = s_w[t];
    a.index[0][p] = s_i[t];
  }
}

// one pass: runs of `width` positions of set `from` merge pairwise into set 1 - from
__global__ __launch_bounds__(kMemThreads) void mem_merge_kernel(MemSortArgs a, uint32_t from, uint64_t width) {
  if (*a.err) return;
  const uint64_t p = (uint64_t)blockIdx.x * kMemThreads + threadIdx.x;
  if (p >= a.n) return;
  const uint64_t* in_w = a.word[from];
  const uint32_t* in_i = a.index[from];
  const uint64_t skip = *a.skip;
  const uint64_t w = in_w[p];
  const uint32_t idx = in_i[p];
  const uint64_t run = p / width, start = run * width, sib = (run ^ 1) * width;
  uint64_t rank = p;
  if (sib < a.n) {  // (else the odd run at the end: it stays where it is)
    uint64_t lo = sib, hi = sib + width < a.n ? sib + width : a.n;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (entry_less(a, skip, in_w[mid], in_i[mid], w, idx)) lo = mid + 1; else hi = mid;
    }
    rank = (start < sib ? start : sib) + (p - start) + (lo - sib);
  }
  if (rank < a.n) {
    a.word[from ^ 1][rank] = w;
    a.index[from ^ 1][rank] = idx;
  }
}

// exclusive sum of v over the workgroup's lanes in lane order, and the total
// (device_common.h's block_excl_sum adds in another order and moves these
// kernels' instructions: this copy stays)
__device__ __forceinline__ void block_excl_scan(uint64_t v, uint64_t* lds, uint64_t& excl, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan(v, lane);
  if (lane == 63) lds[w] = incl;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
  for (uint32_t i = 0; i < (uint32_t)kMemWaves; i++) {
    if (i < w) before += lds[i];
    total += lds[i];
  }
  __syncthreads();  // (the row is free for the caller's next round)
  excl = before + incl - v;
}

// the key length of the entry at sorted position p of set `from` (0 past n)
__device__ __forceinline__ uint64_t sorted_len(const MemSortArgs& a, uint32_t from, uint64_t p, uint32_t& idx) {
  idx = kNoEntry;
  if (p >= a.n) return 0;
  idx = a.index[from][p];
  if (idx >= a.n) return 0;
  return a.key_offsets[idx + 1] - a.key_offsets[idx];
}

__global__ __launch_bounds__(kMemThreads) void mem_len_kernel(MemSortArgs a, uint32_t from) {
  __shared__ uint64_t lds[kMemWaves];
  uint32_t idx;
  const uint64_t len = *a.err ? 0 : sorted_len(a, from, (uint64_t)blockIdx.x * kMemThreads + threadIdx.x, idx);
  uint64_t excl, total;
  block_excl_scan(len, lds, excl, total);
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMemThreads) void mem_scan_kernel(MemSortArgs a) {
  __shared__ uint64_t lds[kMemWaves];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < a.n_tiles; base += kMemThreads) {
    const uint32_t t = base + threadIdx.x;
    const uint64_t v = t < a.n_tiles ? a.tiles[t] : 0;
    uint64_t excl, total;
    block_excl_scan(v, lds, excl, total);
    if (t < a.n_tiles) a.tiles[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const bool bad = *a.err != 0;
    a.counts[0] = bad ? 0 : a.n;
    a.counts[1] = bad ? 0 : carry;
    a.out_key_offsets[bad ? 0 : a.n] = bad ? 0 : carry;  // the slot after the last entry
    a.status[0] = bad ? kMergeBadInput : 0u;
  }
}

__global__ __launch_bounds__(kMemThreads) void mem_emit_kernel(MemSortArgs a, uint32_t from) {
  __shared__ uint64_t lds[kMemWaves];
  if (*a.err) return;  // (uniform)
  const uint64_t p = (uint64_t)blockIdx.x * kMemThreads + threadIdx.x;
  uint32_t idx;
  const uint64_t len = sorted_len(a, from, p, idx);
  uint64_t excl, total;
  block_excl_scan(len, lds, excl, total);
  if (p < a.n) {
    a.source[p] = idx;
    a.out_key_offsets[p] = a.tiles[blockIdx.x] + excl;
  }
}

}  // namespace

hipError_t launch_wb_scan(const WbArgs& a, hipStream_t stream) {
  if (!a.n_records) return hipSuccess;
  const uint64_t wgs = (a.n_records + kMemThreads - 1) / kMemThreads;
  hipLaunchKernelGGL(wb_scan_kernel, dim3((uint32_t)wgs), dim3(kMemThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_wb_decode(const WbArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.max_sequence, 0, sizeof(uint64_t), stream);
  if (e != hipSuccess) return e;
  const uint64_t wgs = a.n_records ? (a.n_records + kMemThreads - 1) / kMemThreads : 1;
  hipLaunchKernelGGL(wb_decode_kernel, dim3((uint32_t)wgs), dim3(kMemThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_memtable_sort(const MemSortArgs& a, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a.err, 0, sizeof(uint32_t), stream);
  if (e == hipSuccess) e = hipMemsetAsync(a.skip, 0xff, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const dim3 grid(a.n_tiles), block(kMemThreads);
  uint32_t from = 0;
  if (a.n) {
    hipLaunchKernelGGL(mem_check_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mem_tile_sort_kernel, grid, block, 0, stream, a);
    for (uint64_t width = kMemThreads; width < a.n; width <<= 1) {
      hipLaunchKernelGGL(mem_merge_kernel, grid, block, 0, stream, a, from, width);
      from ^= 1;
    }
    hipLaunchKernelGGL(mem_len_kernel, grid, block, 0, stream, a, from);
  }
  hipLaunchKernelGGL(mem_scan_kernel, dim3(1), block, 0, stream, a);
  if (a.n) hipLaunchKernelGGL(mem_emit_kernel, grid, block, 0, stream, a, from);
  return hipGetLastError();
}

}  // namespace lsbm
