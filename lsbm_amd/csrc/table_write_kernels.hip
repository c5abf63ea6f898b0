// table_write_kernels.hip -- gfx950 kernels of the batched table finish
// (include/lsbm_table_write.h): what TableBuilder::Finish does between the data
// blocks and the footer for many tables at once, and the memtable sort over
// the memtables of one log.
//
// tw_check_tables_kernel  one lane per word of table_block_first: it begins
//                         with 0, never decreases and ends with n_blocks.
// tw_plan_tile_kernel     one lane per block: WriteBlock's rule, the size that
//                         is kept, size + gap summed over the tile.
// tw_scan_tiles_kernel    one workgroup: running sums over the tiles' totals.
// tw_plan_apply_kernel    one lane per block: its offset, the sum since its
//                         table's first block; one lane per table: its end.
// tw_filter_tile_kernel   one lane per block: does it end a filter (the next
//                         block's offset >> 11 differs, or the table ends), the
//                         filter's first block by a binary search, its bytes;
//                         bytes and filters summed over the tile.
// tw_filter_emit_kernel   one lane per block that ends a filter: filter_first,
//                         filter_out, its slot of the offset array and the
//                         empty slots after it.
// tw_filter_tables_kernel one lane per table: size, count, status, the array
//                         offset and kFilterBaseLg.
// tw_metaindex_kernel     one lane per table: the metaindex block.
// tw_place_kernel         one lane per handle: the table's base added; one
//                         lane per table: its size and its footer.
// seg_check_kernel        one lane per entry: its key's offsets, its segment
//                         (a binary search in seg_first) and how many bytes its
//                         user key shares with its segment's first; one lane
//                         per word of seg_first: the segments tile the entries.
// seg_tile_sort_kernel, seg_merge_kernel, seg_len_kernel, seg_scan_kernel,
// seg_emit_kernel         memtable_kernels.hip's sort with the segment as the
//                         most significant part of the order and the shared
//                         prefix taken per segment.
//
// A block finds its table by a binary search over table_block_first.  What is
// read back from scratch is not trusted: a table found is checked to hold the
// block, a running sum is checked against its window before it addresses a
// byte, an entry index against n.  Every loop halves a range or advances.  No
// spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"       // gcu8, gu8, gptr, gwptr, load8, block_excl_sum, wave_incl_scan
#include "key_compare_device.h"  // bytes_compare
#include "table_write_types.h"

namespace lsbm {
namespace {

constexpr uint32_t kNoEntry = 0xffffffffu;  // the padding of the last sort tile: sorts last
constexpr uint32_t kNoSeg = 0xffffffffu;
constexpr uint32_t kMergeBadInput = 2;      // LSBM_MERGE_BAD_INPUT
constexpr uint64_t kTableMagic = 0xdb4775248b80fb57ull;  // table/format.h:81
constexpr uint32_t kFilterKeyLen = 33;
// "filter." + BloomFilterPolicy::Name()
__constant__ uint8_t kFilterKey[kFilterKeyLen] = {'f', 'i', 'l', 't', 'e', 'r', '.', 'l', 'e', 'v', 'e',
                                                  'l', 'd', 'b', '.', 'B', 'u', 'i', 'l', 't', 'i', 'n',
                                                  'B', 'l', 'o', 'o', 'm', 'F', 'i', 'l', 't', 'e', 'r'};

// ---------------------------------------------------------------- shared

__device__ __forceinline__ uint64_t prefix_a(const TwScan& s, uint64_t i) {
  return i < s.n ? s.a[i] + s.tiles_a[i / kTwThreads] : s.tiles_a[s.n_tiles];
}
__device__ __forceinline__ uint64_t prefix_b(const TwScan& s, uint64_t i) {
  return i < s.n ? s.b[i] + s.tiles_b[i / kTwThreads] : s.tiles_b[s.n_tiles];
}

// the table of block i: the last t with table_block_first[t] <= i, checked to hold i
__device__ __forceinline__ bool find_table(const TwTables& t, uint64_t i, uint64_t& table) {
  if (!t.n_tables) return false;
  uint64_t lo = 0, hi = t.n_tables;
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (t.table_block_first[mid] <= i) lo = mid; else hi = mid;
  }
  table = lo;
  return t.table_block_first[lo] <= i && i < t.table_block_first[lo + 1];
}

__device__ __forceinline__ void put32(uint8_t* out, uint64_t at, uint32_t v) {
  const gu8 p = gwptr(out, at);
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  return v ? (uint32_t)(63 - __builtin_clzll(v)) / 7 + 1 : 1;
}

// PutVarint64 at out[at...); at moves past it
__device__ __forceinline__ void put_varint64(uint8_t* out, uint64_t& at, uint64_t v) {
  while (v >= 128) {
    *gwptr(out, at++) = (uint8_t)(v | 128);
    v >>= 7;
  }
  *gwptr(out, at++) = (uint8_t)v;
}

__global__ __launch_bounds__(kTwThreads) void tw_check_tables_kernel(TwTables t, uint64_t n_blocks, uint32_t* err) {
  const uint64_t j = global_index<kTwThreads>();
  if (j > t.n_tables) return;
  const uint64_t v = t.table_block_first[j];
  const bool bad = (j == 0 && v != 0) || (j == t.n_tables ? v != n_blocks : v > t.table_block_first[j + 1]);
  if (bad) atomicOr(err, 1u);
}

// tiles_x[t] becomes the sum of the tiles before t, tiles_x[n_tiles] the sum of all
__global__ __launch_bounds__(kTwThreads) void tw_scan_tiles_kernel(TwScan s, uint32_t both) {
  __shared__ uint64_t lds[kTwWaves];
  for (uint32_t k = 0; k <= both; k++) {
    uint64_t* tiles = k ? s.tiles_b : s.tiles_a;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < s.n_tiles; base += kTwThreads) {
      const uint64_t t = base + threadIdx.x;
      uint64_t excl, total;
      block_excl_sum<kTwWaves>(t < s.n_tiles ? tiles[t] : 0, lds, excl, total);
      if (t < s.n_tiles) tiles[t] = carry + excl;
      carry += total;
    }
    if (threadIdx.x == 0) tiles[s.n_tiles] = carry;
  }
}

// ---------------------------------------------------------------- the segmented pack plan

__global__ __launch_bounds__(kTwThreads) void tw_plan_tile_kernel(TwPlanArgs a) {
  __shared__ uint64_t lds[kTwWaves];
  if (*a.s.err) return;  // (uniform)
  const uint64_t i = global_index<kTwThreads>();
  uint64_t size = 0, v = 0;
  uint32_t type = 0;
  if (i < a.s.n) {
    const uint64_t raw = a.raw_len[i];
    const uint64_t comp = a.comp_len ? a.comp_len[i] : UINT64_MAX;
    // compressed.size() < raw.size() - raw.size() / 8 (table/table_builder.cc:187)
    type = (comp != UINT64_MAX && comp < raw - raw / 8) ? 1u : 0u;
    size = type ? comp : raw;
    v = size + a.gap;
  }
  uint64_t excl, total;
  block_excl_sum<kTwWaves>(v, lds, excl, total);
  if (i < a.s.n) {
    a.types[i] = (uint8_t)type;
    a.handles[2 * i + 1] = size;
    a.s.a[i] = excl;
  }
  if (threadIdx.x == 0) a.s.tiles_a[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTwThreads) void tw_plan_apply_kernel(TwPlanArgs a) {
  const uint64_t j = global_index<kTwThreads>();
  const bool bad = *a.s.err != 0;
  if (j < a.s.n) {
    uint64_t t;
    if (bad || !find_table(a.t, j, t)) return;
    const uint64_t first = a.first_offset ? a.first_offset[t] : 0;
    a.handles[2 * j] = first + prefix_a(a.s, j) - prefix_a(a.s, a.t.table_block_first[t]);
  } else if (j - a.s.n < a.t.n_tables) {
    const uint64_t t = j - a.s.n;
    if (!bad) {
      const uint64_t first = a.first_offset ? a.first_offset[t] : 0;
      a.end[t] = first + prefix_a(a.s, a.t.table_block_first[t + 1]) - prefix_a(a.s, a.t.table_block_first[t]);
    }
    a.status[t] = bad ? kTwBadInput : kTwOk;
  }
}

// ---------------------------------------------------------------- the filter block's layout

// What block i of table t (it holds i) means to FilterBlockBuilder.
struct TwGroup {
  bool ends;         // a filter is generated after this block
  uint64_t g0;       // the filter's first block
  uint64_t keys;     // its keys
  uint64_t bytes;    // CreateFilter's bytes for them (0 without a key)
  uint64_t fi;       // its slot of the offset array
  uint64_t next_fi;  // the slot of the filter after it (the table's end: data_end >> 11)
};

__device__ __forceinline__ TwGroup filter_group(const TwFilterArgs& a, uint64_t i, uint64_t t) {
  TwGroup g = {};
  const uint64_t b0 = a.t.table_block_first[t], b1 = a.t.table_block_first[t + 1];
  g.fi = a.data_handles[2 * i] >> kTwFilterBaseLg;
  g.next_fi = (i + 1 == b1 ? a.data_end[t] : a.data_handles[2 * (i + 1)]) >> kTwFilterBaseLg;
  g.ends = i + 1 == b1 || g.next_fi != g.fi;
  if (!g.ends) return g;
  // the first block of [b0, i] whose slot is fi (offsets never decrease inside a table)
  uint64_t lo = b0, hi = i;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((a.data_handles[2 * mid] >> kTwFilterBaseLg) >= g.fi) hi = mid; else lo = mid + 1;
  }
  g.g0 = lo;
  const uint64_t k0 = a.block_first[lo], k1 = a.block_first[i + 1];
  g.keys = k1 > k0 ? k1 - k0 : 0;
  if (g.keys) {
    uint64_t bits = g.keys * a.bits_per_key;  // util/bloom.cc:39-46
    if (bits < 64) bits = 64;
    g.bytes = (bits + 7) / 8 + 1;  // + the k byte (:50)
  }
  return g;
}

// a table's filter data bytes and the slots of its offset array
__device__ __forceinline__ void filter_table(const TwFilterArgs& a, uint64_t t, uint64_t& data_bytes, uint64_t& slots) {
  const uint64_t b0 = a.t.table_block_first[t], b1 = a.t.table_block_first[t + 1];
  data_bytes = prefix_a(a.s, b1) - prefix_a(a.s, b0);
  slots = 0;
  if (b1 > b0) {
    const uint64_t fi_last = a.data_handles[2 * (b1 - 1)] >> kTwFilterBaseLg, fi_end = a.data_end[t] >> kTwFilterBaseLg;
    slots = fi_end + (fi_end == fi_last ? 1 : 0);
  }
}

// the table's window holds its filter block (and every filter of the call has a slot)
__device__ __forceinline__ bool filter_fits(const TwFilterArgs& a, uint64_t t, uint64_t data_bytes, uint64_t slots,
                                            uint64_t& off) {
  off = a.out_handles[2 * t];
  const uint64_t size = a.out_handles[2 * t + 1], need = data_bytes + 4 * slots + 5;
  return off <= a.out_size && size <= a.out_size - off && need <= size && data_bytes <= need &&
         prefix_b(a.s, a.s.n) <= a.filters_cap;
}

__global__ __launch_bounds__(kTwThreads) void tw_filter_tile_kernel(TwFilterArgs a) {
  __shared__ uint64_t lds[kTwWaves];
  if (*a.s.err) return;  // (uniform)
  const uint64_t i = global_index<kTwThreads>();
  uint64_t bytes = 0, count = 0, t;
  if (i < a.s.n && find_table(a.t, i, t)) {
    const TwGroup g = filter_group(a, i, t);
    if (g.ends && g.keys) bytes = g.bytes, count = 1;
  }
  uint64_t excl, total;
  block_excl_sum<kTwWaves>(bytes, lds, excl, total);
  if (i < a.s.n) a.s.a[i] = excl;
  if (threadIdx.x == 0) a.s.tiles_a[blockIdx.x] = total;
  block_excl_sum<kTwWaves>(count, lds, excl, total);
  if (i < a.s.n) a.s.b[i] = excl;
  if (threadIdx.x == 0) a.s.tiles_b[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTwThreads) void tw_filter_emit_kernel(TwFilterArgs a) {
  if (*a.s.err) return;
  const uint64_t i = global_index<kTwThreads>();
  uint64_t t;
  if (i >= a.s.n || !find_table(a.t, i, t)) return;
  const TwGroup g = filter_group(a, i, t);
  if (!g.ends) return;
  uint64_t data_bytes, slots, off;
  filter_table(a, t, data_bytes, slots);
  const bool fits = filter_fits(a, t, data_bytes, slots, off);
  const uint64_t rel = prefix_a(a.s, i) - prefix_a(a.s, a.t.table_block_first[t]);
  if (g.keys) {
    const uint64_t f = prefix_b(a.s, i);
    if (f < a.filters_cap) {
      a.filter_first[f] = a.block_first[g.g0];
      a.filter_out[f] = fits && rel <= data_bytes && g.bytes <= data_bytes - rel ? off + rel : kTwNoPlace;
    }
  }
  if (!fits) return;
  // the filter's slot, and the empty ones up to the next filter's: GenerateFilter without keys
  const uint64_t array = off + data_bytes;
  if (g.fi < slots) put32(a.out, array + 4 * g.fi, (uint32_t)rel);
  const uint64_t stop = g.next_fi < slots ? g.next_fi : slots;
  for (uint64_t s = g.fi + 1; s < stop; s++) put32(a.out, array + 4 * s, (uint32_t)(rel + g.bytes));
}

__global__ __launch_bounds__(kTwThreads) void tw_filter_tables_kernel(TwFilterArgs a) {
  const uint64_t t = global_index<kTwThreads>();
  if (t >= a.t.n_tables) return;
  if (*a.s.err) {
    a.status[t] = kTwBadInput;
    return;
  }
  uint64_t data_bytes, slots;
  filter_table(a, t, data_bytes, slots);
  a.filter_size[t] = data_bytes + 4 * slots + 5;
  a.filter_count[t] = prefix_b(a.s, a.t.table_block_first[t + 1]) - prefix_b(a.s, a.t.table_block_first[t]);
  uint32_t st = kTwOk;
  if (a.out) {
    uint64_t off;
    if (filter_fits(a, t, data_bytes, slots, off)) {
      put32(a.out, off + data_bytes + 4 * slots, (uint32_t)data_bytes);
      *gwptr(a.out, off + data_bytes + 4 * slots + 4) = (uint8_t)kTwFilterBaseLg;
    } else {
      st = kTwNoRoom;
    }
    const uint64_t filters = prefix_b(a.s, a.s.n);
    if (t == 0 && filters <= a.filters_cap) a.filter_first[filters] = a.block_first[a.s.n];
  }
  a.status[t] = st;
}

// ---------------------------------------------------------------- the metaindex block

__global__ __launch_bounds__(kTwThreads) void tw_metaindex_kernel(TwMetaArgs a) {
  const uint64_t t = global_index<kTwThreads>();
  if (t >= a.n_tables) return;
  const bool with = a.filter_size != nullptr;
  const uint64_t h_off = a.data_end[t], h_size = with ? a.filter_size[t] : 0;
  const uint32_t value_len = varint_len(h_off) + varint_len(h_size);
  // shared, non_shared, value_length, the key, the value; one restart and their count
  const uint64_t need = with ? 3 + kFilterKeyLen + value_len + 8 : 8;
  a.sizes[t] = need;
  uint32_t st = kTwOk;
  if (a.out) {
    const uint64_t off = a.out_handles[2 * t], size = a.out_handles[2 * t + 1];
    if (off <= a.out_size && size <= a.out_size - off && need <= size) {
      uint64_t at = off;
      if (with) {
        *gwptr(a.out, at++) = 0;
        *gwptr(a.out, at++) = (uint8_t)kFilterKeyLen;
        *gwptr(a.out, at++) = (uint8_t)value_len;
        for (uint32_t k = 0; k < kFilterKeyLen; k++) *gwptr(a.out, at++) = kFilterKey[k];
        put_varint64(a.out, at, h_off);  // BlockHandle::EncodeTo
        put_varint64(a.out, at, h_size);
      }
      put32(a.out, at, 0);
      put32(a.out, at + 4, 1);
    } else {
      st = kTwNoRoom;
    }
  }
  a.status[t] = st;
}

// ---------------------------------------------------------------- footers and placement

__global__ __launch_bounds__(kTwThreads) void tw_place_kernel(TwPlaceArgs a) {
  const uint64_t j = global_index<kTwThreads>();
  const bool bad = *a.err != 0;
  const uint64_t n_tail = (uint64_t)a.tail_per_table * a.t.n_tables;
  if (j < a.n) {
    uint64_t t;
    if (bad || !find_table(a.t, j, t)) return;
    a.abs_data_handles[2 * j] = a.data_handles[2 * j] + a.table_base[t];
    a.abs_data_handles[2 * j + 1] = a.data_handles[2 * j + 1];
  } else if (j - a.n < n_tail) {
    if (bad) return;
    const uint64_t k = j - a.n, t = k / a.tail_per_table;
    a.abs_tail_handles[2 * k] = a.tail_handles[2 * k] + a.table_base[t];
    a.abs_tail_handles[2 * k + 1] = a.tail_handles[2 * k + 1];
  } else if (j - a.n - n_tail < a.t.n_tables) {
    const uint64_t t = j - a.n - n_tail;
    if (bad) {
      a.status[t] = kTwBadInput;
      return;
    }
    const uint64_t end = a.tail_end[t], base = a.table_base[t], size = end + kTwFooterBytes;
    a.table_size[t] = size;
    if (size < end || base > a.arena_size || size > a.arena_size - base) {
      a.status[t] = kTwNoRoom;
      return;
    }
    // Footer::EncodeTo: the metaindex and the index handle, zeros up to 40 bytes, the magic
    const uint64_t* h = a.tail_handles + 2 * ((t + 1) * a.tail_per_table - 2);
    const uint64_t at0 = base + end;
    uint64_t at = at0;
    for (uint32_t k = 0; k < 4; k++) put_varint64(a.arena, at, h[k]);
    while (at < at0 + 40) *gwptr(a.arena, at++) = 0;
    put32(a.arena, at0 + 40, (uint32_t)kTableMagic);
    put32(a.arena, at0 + 44, (uint32_t)(kTableMagic >> 32));
    a.status[t] = kTwOk;
  }
}

// ---------------------------------------------------------------- the segmented sort

// bytes the user keys at [ka, ka + ua) and [kb, kb + ub) have in common at their start
__device__ __forceinline__ uint64_t common_prefix(const SegSortArgs& a, uint64_t ka, uint64_t ua, uint64_t kb,
                                                  uint64_t ub) {
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

__device__ __forceinline__ bool key_ok(const SegSortArgs& a, uint64_t ka, uint64_t kb) {
  return ka <= kb && kb <= a.keys_size && kb - ka >= 8;
}

__global__ __launch_bounds__(kTwThreads) void seg_check_kernel(SegSortArgs a) {
  const uint64_t j = global_index<kTwThreads>();
  if (j <= a.n_segs) {
    const uint64_t v = a.seg_first[j];
    if ((j == 0 && v != 0) || (j == a.n_segs ? v != a.n : v > a.seg_first[j + 1])) atomicOr(a.err, 1u);
  }
  uint32_t shared = 0xffffffffu, seg = kNoSeg;  // with its segment's first user key
  if (j < a.n) {
    const uint64_t ka = a.key_offsets[j], kb = a.key_offsets[j + 1];
    uint64_t lo = 0, hi = a.n_segs;
    while (hi - lo > 1) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (a.seg_first[mid] <= j) lo = mid; else hi = mid;
    }
    if (!key_ok(a, ka, kb) || !a.n_segs || lo > 0xfffffffeull || a.seg_first[lo] > j || a.seg_first[lo + 1] <= j) {
      atomicOr(a.err, 1u);
    } else {
      seg = (uint32_t)lo;
      a.seg[j] = seg;
      const uint64_t z = a.seg_first[lo];  // (<= j: an entry)
      const uint64_t za = a.key_offsets[z], zb = a.key_offsets[z + 1];
      if (key_ok(a, za, zb)) {  // (else that entry's own lane reports it)
        const uint64_t c = common_prefix(a, ka, kb - ka - 8, za, zb - za - 8);
        shared = c < 0xffffffffu ? (uint32_t)c : 0xfffffffeu;
      }
    }
  }
  // a wave inside one segment: one atomic for all of it
  const uint32_t seg0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg);
  if (__ballot(seg != seg0) == 0) {
    for (uint32_t o = 32; o > 0; o >>= 1) {
      const uint32_t other = __shfl_xor(shared, o);
      shared = other < shared ? other : shared;
    }
    if ((threadIdx.x & 63) == 0 && seg0 != kNoSeg && shared != 0xffffffffu) atomicMin(a.skip + seg0, shared);
  } else if (seg != kNoSeg && shared != 0xffffffffu) {
    atomicMin(a.skip + seg, shared);
  }
}

// the sort word of the key at [ka, ka + klen), klen >= 8, when every user key
// of its segment starts with the same `skip` bytes (memtable_kernels.hip)
__device__ __forceinline__ uint64_t sort_word(const SegSortArgs& a, uint64_t ka, uint64_t klen, uint64_t skip) {
  const uint64_t ulen = klen - 8, at = skip < ulen ? skip : ulen, rest = ulen - at;
  const uint64_t be = __builtin_bswap64(load8(gptr(a.keys, ka + at)));  // (8 bytes of the key: klen - at >= 8)
  const uint32_t take = rest < 7 ? (uint32_t)rest : 7;
  const uint64_t mask = take ? ~0ull << (64 - 8 * take) : 0;
  return (be & mask) | (rest < 8 ? rest : 8);
}

__device__ __forceinline__ uint32_t seg_of(const SegSortArgs& a, uint32_t idx) {
  return idx < a.n ? a.seg[idx] : kNoSeg;
}

// entry ia (segment sa, word wa) comes before entry ib: the segment first, then
// the memtable's order: user key ascending, tag descending, later arrival first
__device__ __forceinline__ bool entry_less(const SegSortArgs& a, uint32_t sa, uint64_t wa, uint32_t ia, uint32_t sb,
                                           uint64_t wb, uint32_t ib) {
  if (sa != sb) return sa < sb;
  if (wa != wb) return wa < wb;
  if (ia == ib || ia >= a.n || ib >= a.n || sa >= a.n_segs) return false;  // (padding, or scratch that is not trusted)
  const uint64_t ka = a.key_offsets[ia], la = a.key_offsets[ia + 1] - ka;
  const uint64_t kb = a.key_offsets[ib], lb = a.key_offsets[ib + 1] - kb;
  const uint64_t done = (uint64_t)a.skip[sa] + 7;  // user-key bytes the equal words stand for
  if ((wa & 0xff) == 8 && la >= done + 9 && lb >= done + 9) {  // (8 there: a user key of skip + 8 bytes or more)
    const int c = bytes_compare(gptr(a.keys, ka + done), la - 8 - done, gptr(a.keys, kb + done), lb - 8 - done);
    if (c) return c < 0;
  }
  const uint64_t ta = load8(gptr(a.keys, ka + la - 8)), tb = load8(gptr(a.keys, kb + lb - 8));
  if (ta != tb) return ta > tb;
  return ia > ib;
}

__global__ __launch_bounds__(kTwThreads) void seg_tile_sort_kernel(SegSortArgs a) {
  __shared__ uint64_t s_w[kTwThreads];
  __shared__ uint32_t s_i[kTwThreads];
  __shared__ uint32_t s_s[kTwThreads];
  if (*a.err) return;  // (uniform)
  const uint32_t t = threadIdx.x, p = blockIdx.x * kTwThreads + t;
  uint64_t w = ~0ull;
  uint32_t idx = kNoEntry, seg = kNoSeg;
  if (p < a.n) {
    const uint32_t s = a.seg[p];
    if (s < a.n_segs) {  // (else scratch that is not trusted: the entry sorts last)
      const uint64_t ka = a.key_offsets[p];
      w = sort_word(a, ka, a.key_offsets[p + 1] - ka, a.skip[s]);
      seg = s;
    }
    idx = p;
  }
  s_w[t] = w;
  s_i[t] = idx;
  s_s[t] = seg;
  for (uint32_t k = 2; k <= (uint32_t)kTwThreads; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const uint32_t q = t ^ j;
      if (q > t) {
        const uint64_t w0 = s_w[t], w1 = s_w[q];
        const uint32_t i0 = s_i[t], i1 = s_i[q], g0 = s_s[t], g1 = s_s[q];
        const bool up = (t & k) == 0;
        if (up ? entry_less(a, g1, w1, i1, g0, w0, i0) : entry_less(a, g0, w0, i0, g1, w1, i1)) {
          s_w[t] = w1;
          s_i[t] = i1;
          s_s[t] = g1;
          s_w[q] = w0;
          s_i[q] = i0;
          s_s[q] = g0;
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
__global__ __launch_bounds__(kTwThreads) void seg_merge_kernel(SegSortArgs a, uint32_t from, uint64_t width) {
  if (*a.err) return;
  const uint64_t p = global_index<kTwThreads>();
  if (p >= a.n) return;
  const uint64_t* in_w = a.word[from];
  const uint32_t* in_i = a.index[from];
  const uint64_t w = in_w[p];
  const uint32_t idx = in_i[p], seg = seg_of(a, idx);
  const uint64_t run = p / width, start = run * width, sib = (run ^ 1) * width;
  uint64_t rank = p;
  if (sib < a.n) {  // (else the odd run at the end: it stays where it is)
    uint64_t lo = sib, hi = sib + width < a.n ? sib + width : a.n;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      const uint32_t mi = in_i[mid];
      if (entry_less(a, seg_of(a, mi), in_w[mid], mi, seg, w, idx)) lo = mid + 1; else hi = mid;
    }
    rank = (start < sib ? start : sib) + (p - start) + (lo - sib);
  }
  if (rank < a.n) {
    a.word[from ^ 1][rank] = w;
    a.index[from ^ 1][rank] = idx;
  }
}

// the key length of the entry at sorted position p of set `from` (0 past n)
__device__ __forceinline__ uint64_t sorted_len(const SegSortArgs& a, uint32_t from, uint64_t p, uint32_t& idx) {
  idx = kNoEntry;
  if (p >= a.n) return 0;
  idx = a.index[from][p];
  if (idx >= a.n) return 0;
  return a.key_offsets[idx + 1] - a.key_offsets[idx];
}

__global__ __launch_bounds__(kTwThreads) void seg_len_kernel(SegSortArgs a, uint32_t from) {
  __shared__ uint64_t lds[kTwWaves];
  uint32_t idx;
  const uint64_t len = *a.err ? 0 : sorted_len(a, from, global_index<kTwThreads>(), idx);
  uint64_t excl, total;
  block_excl_sum<kTwWaves>(len, lds, excl, total);
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTwThreads) void seg_scan_kernel(SegSortArgs a) {
  __shared__ uint64_t lds[kTwWaves];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < a.n_tiles; base += kTwThreads) {
    const uint32_t t = base + threadIdx.x;
    const uint64_t v = t < a.n_tiles ? a.tiles[t] : 0;
    uint64_t excl, total;
    block_excl_sum<kTwWaves>(v, lds, excl, total);
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

__global__ __launch_bounds__(kTwThreads) void seg_emit_kernel(SegSortArgs a, uint32_t from) {
  __shared__ uint64_t lds[kTwWaves];
  if (*a.err) return;  // (uniform)
  const uint64_t p = global_index<kTwThreads>();
  uint32_t idx;
  const uint64_t len = sorted_len(a, from, p, idx);
  uint64_t excl, total;
  block_excl_sum<kTwWaves>(len, lds, excl, total);
  if (p < a.n) {
    a.source[p] = idx;
    a.out_key_offsets[p] = a.tiles[blockIdx.x] + excl;
  }
}

uint32_t wgs_of(uint64_t lanes) { return (uint32_t)((lanes + kTwThreads - 1) / kTwThreads); }

hipError_t check_tables(const TwTables& t, uint64_t n_blocks, uint32_t* err, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(err, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tw_check_tables_kernel, dim3(wgs_of(t.n_tables + 1)), dim3(kTwThreads), 0, stream, t, n_blocks,
                     err);
  return hipSuccess;
}

}  // namespace

hipError_t launch_table_pack_plan(const TwPlanArgs& a, hipStream_t stream) {
  const hipError_t e = check_tables(a.t, a.s.n, a.s.err, stream);
  if (e != hipSuccess) return e;
  const dim3 block(kTwThreads);
  if (a.s.n) hipLaunchKernelGGL(tw_plan_tile_kernel, dim3((uint32_t)a.s.n_tiles), block, 0, stream, a);
  hipLaunchKernelGGL(tw_scan_tiles_kernel, dim3(1), block, 0, stream, a.s, 0u);
  if (a.s.n + a.t.n_tables)
    hipLaunchKernelGGL(tw_plan_apply_kernel, dim3(wgs_of(a.s.n + a.t.n_tables)), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_filter_layout(const TwFilterArgs& a, hipStream_t stream) {
  const hipError_t e = check_tables(a.t, a.s.n, a.s.err, stream);
  if (e != hipSuccess) return e;
  const dim3 block(kTwThreads), grid((uint32_t)a.s.n_tiles);
  if (a.s.n) hipLaunchKernelGGL(tw_filter_tile_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(tw_scan_tiles_kernel, dim3(1), block, 0, stream, a.s, 1u);
  if (a.s.n && a.out) hipLaunchKernelGGL(tw_filter_emit_kernel, grid, block, 0, stream, a);
  if (a.t.n_tables) hipLaunchKernelGGL(tw_filter_tables_kernel, dim3(wgs_of(a.t.n_tables)), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_metaindex(const TwMetaArgs& a, hipStream_t stream) {
  if (!a.n_tables) return hipSuccess;
  hipLaunchKernelGGL(tw_metaindex_kernel, dim3(wgs_of(a.n_tables)), dim3(kTwThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_table_place(const TwPlaceArgs& a, hipStream_t stream) {
  const hipError_t e = check_tables(a.t, a.n, a.err, stream);
  if (e != hipSuccess) return e;
  const uint64_t lanes = a.n + ((uint64_t)a.tail_per_table + 1) * a.t.n_tables;
  if (lanes) hipLaunchKernelGGL(tw_place_kernel, dim3(wgs_of(lanes)), dim3(kTwThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sort_segments(const SegSortArgs& a, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a.err, 0, sizeof(uint32_t), stream);
  if (e == hipSuccess && a.n_segs) e = hipMemsetAsync(a.skip, 0xff, sizeof(uint32_t) * a.n_segs, stream);
  if (e != hipSuccess) return e;
  const dim3 grid(a.n_tiles), block(kTwThreads);
  uint32_t from = 0;
  const uint64_t checks = a.n > a.n_segs + 1 ? a.n : a.n_segs + 1;
  hipLaunchKernelGGL(seg_check_kernel, dim3(wgs_of(checks)), block, 0, stream, a);
  if (a.n) {
    hipLaunchKernelGGL(seg_tile_sort_kernel, grid, block, 0, stream, a);
    for (uint64_t width = kTwThreads; width < a.n; width <<= 1) {
      hipLaunchKernelGGL(seg_merge_kernel, grid, block, 0, stream, a, from, width);
      from ^= 1;
    }
    hipLaunchKernelGGL(seg_len_kernel, grid, block, 0, stream, a, from);
  }
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), block, 0, stream, a);
  if (a.n) hipLaunchKernelGGL(seg_emit_kernel, grid, block, 0, stream, a, from);
  return hipGetLastError();
}

}  // namespace lsbm
