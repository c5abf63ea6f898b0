// block_build_kernels.hip -- gfx950 kernels of the batched SSTable block
// builder (include/lsbm_block_build.h): BlockBuilder::Add / Finish of
// table/block_builder.cc, TableBuilder::Add's flush rule and the index block.
//
// plan_sizes_kernel   one lane per entry: its encoded size with the prefix it
//                     shares with its predecessor, and as a restart point.
// plan_links_kernel   one lane per entry: "if a block started here, how many
//                     entries would it hold and what would Finish() return" --
//                     a walk over the sizes above, no key byte read.
// plan_chain_kernel   one wave per table: lane 0 follows the links, staged in
//                     LDS kPlanChunk at a time; the wave sizes the table's
//                     last block (cut by the table's end, not by the rule).
// plan_scan_kernel    one wave: running block count over the tables.
// plan_emit_kernel    one workgroup per table: block_first / block_bytes, dense.
// block_build_kernel  one wave per block: the lanes size 64 entries at a time
//                     (an entry's shared prefix depends only on its
//                     predecessor's key), prefix-sum the sizes, each lane
//                     writes its entry's header and restart slot, and all 64
//                     lanes copy each entry's key delta and value.
// index_build_kernel  one wave per table, one lane per data block: separator
//                     or successor, BlockHandle, at restart interval 1 every
//                     entry is independent of its predecessor.
//
// A block of at most kBuildTileBytes is assembled in the wave's LDS tile, which
// keeps the 16-B phase of its window, and leaves with aligned 16-B stores; a
// larger one is written straight to global memory by the same code, templated
// on the pointer type.
//
// Every offset and length of the input is untrusted: a key's bounds are
// checked against keys_size and a value slice against the value image before
// a byte is read, a block's size against its window (and the window against
// the output) before a byte is written.  No spin-waits, no cross-workgroup
// state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_build_types.h"
#include "device_common.h"  // gcu8, gu8, lu8, u32x4, gu32x4, gptr, gwptr, wave_phase, wave_sum, wave_incl_scan

namespace lsbm {
namespace {

typedef const __attribute__((address_space(3))) u32x4* lcu32x4;

constexpr uint32_t kSizeTooLarge = 0xffffffffu;  // plan: an entry of 2^32 - 1 bytes or more
constexpr uint32_t kSizeBad = 0xfffffffeu;       // plan: an entry whose key offsets are bad
constexpr uint64_t kBytesBad = ~0ull;            // plan: a block with such an entry
constexpr uint64_t kBytesTooLarge = ~0ull - 1;
constexpr uint64_t kMaxBlock = 1ull << 32;

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o);
    v = t > v ? t : v;
  }
  return v;
}
// lane q's value in every lane (q uniform)
__device__ __forceinline__ uint32_t bcast32(uint32_t v, uint32_t q) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)q);
}
__device__ __forceinline__ uint64_t bcast64(uint64_t v, uint32_t q) {
  return (uint64_t)bcast32((uint32_t)v, q) | ((uint64_t)bcast32((uint32_t)(v >> 32), q) << 32);
}

__device__ __forceinline__ uint32_t varint_len(uint64_t v) {  // util/coding.cc:VarintLength
  uint32_t n = 1;
  while (v >= 128) {
    v >>= 7;
    n++;
  }
  return n;
}

template <class P>
__device__ __forceinline__ uint64_t put_varint(P d, uint64_t p, uint64_t v) {  // PutVarint32 / 64
  while (v >= 128) {
    d[p++] = (uint8_t)(v | 128);
    v >>= 7;
  }
  d[p++] = (uint8_t)v;
  return p;
}

template <class P>
__device__ __forceinline__ void put_le32(P d, uint64_t p, uint32_t v) {  // EncodeFixed32, any alignment
  d[p] = (uint8_t)v;
  d[p + 1] = (uint8_t)(v >> 8);
  d[p + 2] = (uint8_t)(v >> 16);
  d[p + 3] = (uint8_t)(v >> 24);
}

// length of the common prefix of a[0, alen) and b[0, blen)
__device__ __forceinline__ uint64_t common_prefix(gcu8 a, uint64_t alen, gcu8 b, uint64_t blen) {
  const uint64_t m = alen < blen ? alen : blen;
  uint64_t i = 0;
  // eight bytes at a step while both keys have them (each step waits for its
  // two loads: a 31-byte key is 4 steps this way, 24+ a byte at a time)
  while (i + 8 <= m) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + i, 8);
    __builtin_memcpy(&y, b + i, 8);
    if (x != y) return i + ((uint64_t)__builtin_ctzll(x ^ y) >> 3);  // little-endian: the lowest differing byte
    i += 8;
  }
  while (i < m && a[i] == b[i]) i++;
  return i;
}

// key j's bounds: false if its offsets decrease or pass keys_size
__device__ __forceinline__ bool key_of(const BuildEntries& e, uint64_t j, uint64_t& a, uint64_t& len) {
  a = e.key_offsets[j];
  const uint64_t b = e.key_offsets[j + 1];
  len = b - a;
  return a <= b && b <= e.keys_size;
}

// (an entry within 8 bytes of 2^32 makes its block too large whatever else it holds)
__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v >= kSizeBad ? kSizeTooLarge : (uint32_t)v; }

// ---------------------------------------------------------------- plan

__global__ __launch_bounds__(kBuildThreads) void plan_sizes_kernel(PlanArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBuildThreads;
  for (uint64_t j = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x; j < a.e.n; j += stride) {
    uint64_t ka, klen;
    uint32_t ss = kSizeBad, sr = kSizeBad;
    if (key_of(a.e, j, ka, klen)) {
      const uint64_t vlen = a.e.values[2 * j + 1];
      uint64_t shared = 0, pa, plen;
      if (j > 0 && key_of(a.e, j - 1, pa, plen)) shared = common_prefix(gptr(a.e.keys, pa), plen, gptr(a.e.keys, ka), klen);
      const uint64_t vl = varint_len(vlen);
      // (vlen up to 2^64 - 1: the sums saturate instead of wrapping)
      const uint64_t body_r = 1 + varint_len(klen) + vl + klen, body_s = varint_len(shared) + varint_len(klen - shared) + vl + (klen - shared);
      sr = vlen > ~0ull - body_r ? kSizeTooLarge : sat32(body_r + vlen);
      ss = vlen > ~0ull - body_s ? kSizeTooLarge : sat32(body_s + vlen);
    }
    a.s.sizes[2 * j] = ss;
    a.s.sizes[2 * j + 1] = sr;
  }
}

// The running state of one BlockBuilder over the planned sizes.
struct PlanWalk {
  uint64_t buf, restarts;
  uint32_t counter;
  bool bad, large;
  __device__ __forceinline__ void reset() {
    buf = 0;
    restarts = 1;
    counter = 0;
    bad = large = false;
  }
  // Add(entry j) as position `first ? 0 : later` of the block (table/block_builder.cc:75-107)
  __device__ __forceinline__ void add(const uint32_t* sizes, uint64_t j, uint32_t interval, bool first) {
    uint32_t s;
    if (first || counter >= interval) {
      if (!first) restarts++;
      counter = 0;
      s = sizes[2 * j + 1];
    } else {
      s = sizes[2 * j];
    }
    bad |= s == kSizeBad;
    large |= s == kSizeTooLarge;
    buf += s;
    counter++;
  }
  __device__ __forceinline__ uint64_t estimate() const { return buf + 4 * restarts + 4; }  // CurrentSizeEstimate
  __device__ __forceinline__ uint64_t bytes() const {
    if (bad) return kBytesBad;
    return (large || estimate() >= kMaxBlock) ? kBytesTooLarge : estimate();
  }
};

__global__ __launch_bounds__(kBuildThreads) void plan_links_kernel(PlanArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBuildThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x; i < a.e.n; i += stride) {
    PlanWalk w;
    w.reset();
    uint64_t j = i;
    do {
      w.add(a.s.sizes, j, a.restart_interval, j == i);
      j++;
    } while (j < a.e.n && w.estimate() < a.block_size);
    a.s.link[i] = j - i;
    a.s.bytes[i] = w.bytes();
  }
}

__device__ __forceinline__ uint32_t bytes_status(uint64_t bytes) {
  return bytes == kBytesBad ? kBuildBadInput : (bytes == kBytesTooLarge ? kBuildTooLarge : kBuildOk);
}

__global__ __launch_bounds__(kBuildThreads) void plan_chain_kernel(PlanArgs a) {
  __shared__ uint64_t links[kBuildWaves][kPlanChunk];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t stride = (uint64_t)gridDim.x * kBuildWaves;
  for (uint64_t t = (uint64_t)blockIdx.x * kBuildWaves + wv; t < a.n_tables; t += stride) {
    const uint64_t t0 = a.table_first[t], t1 = a.table_first[t + 1];
    if (t0 > t1 || t1 > a.e.n) {
      if (lane == 0) {
        a.s.counts[t] = 0;
        a.s.last[t] = 0;
        a.status[t] = kBuildBadInput;
      }
      continue;
    }
    uint64_t cur = t0, nb = 0, last = t0;
    while (cur < t1) {
      const uint64_t c0 = cur, cn = t1 - c0 < kPlanChunk ? t1 - c0 : kPlanChunk;
      for (uint64_t i = lane; i < cn; i += 64) links[wv][i] = a.s.link[c0 + i];
      wave_phase();
      if (lane == 0) {
        while (cur - c0 < cn) {  // (a link is at least 1)
          a.s.starts[t0 + nb] = cur;
          last = cur;
          nb++;
          cur += links[wv][cur - c0];
        }
      }
      cur = bcast64(cur, 0);
      nb = bcast64(nb, 0);
      last = bcast64(last, 0);
      wave_phase();
    }
    // the table's last block [last, t1): what is left, not what the rule cuts
    uint64_t bytes = 0;
    if (nb) {
      const uint64_t n = t1 - last, ri = a.restart_interval;
      uint64_t sum = 0;
      uint32_t flag = 0;
      for (uint64_t k = lane; k < n; k += 64) {
        const uint32_t s = a.s.sizes[2 * (last + k) + (k % ri == 0 ? 1 : 0)];
        flag |= s == kSizeBad ? 2u : (s == kSizeTooLarge ? 1u : 0u);
        sum += s;
      }
      sum = wave_sum(sum);
      flag = wave_max(flag);  // (bad input outranks too large only within one block's verdict below)
      const uint64_t fin = sum + 4 * ((n + ri - 1) / ri) + 4;
      bytes = (flag & 2u) ? kBytesBad : ((flag || fin >= kMaxBlock) ? kBytesTooLarge : fin);
    }
    if (lane == 0) {
      a.s.counts[t] = nb;
      a.s.last[t] = bytes;
      a.status[t] = bytes_status(bytes);
    }
  }
}

__global__ __launch_bounds__(64) void plan_scan_kernel(PlanArgs a) {
  const uint32_t lane = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t c = 0; c < a.n_tables; c += 64) {
    const uint64_t t = c + lane, v = t < a.n_tables ? a.s.counts[t] : 0;
    const uint64_t inc = wave_incl_scan(v, lane);
    if (t < a.n_tables) a.table_block_first[t] = carry + inc - v;
    carry += bcast64(inc, 63);
  }
  if (lane == 0) {
    a.table_block_first[a.n_tables] = carry;
    if (carry <= a.blocks_cap) {  // the end, in the slot after the last block
      const uint64_t end = a.table_first[a.n_tables];
      a.block_first[carry] = end < a.e.n ? end : a.e.n;
    }
  }
}

__global__ __launch_bounds__(kBuildThreads) void plan_emit_kernel(PlanArgs a) {
  for (uint64_t t = blockIdx.x; t < a.n_tables; t += gridDim.x) {
    const uint64_t nb = a.s.counts[t], b0 = a.table_block_first[t], t0 = a.table_first[t];
    uint32_t worst = kBuildOk;
    for (uint64_t lb = threadIdx.x; lb < nb; lb += kBuildThreads) {
      const uint64_t s = a.s.starts[t0 + lb], b = b0 + lb;
      const uint64_t bytes = lb + 1 == nb ? a.s.last[t] : a.s.bytes[s];
      const uint32_t st = bytes_status(bytes);
      worst = st > worst ? st : worst;
      if (b <= a.blocks_cap) a.block_first[b] = s;
      if (b < a.blocks_cap) a.block_bytes[b] = st == kBuildOk ? bytes : 0;
    }
    if (worst != kBuildOk) atomicMax(&a.status[t], worst);
  }
}

// ---------------------------------------------------------------- build

// The finished block in the wave's tile (at the window's 16-B phase) -> global.
__device__ __forceinline__ void flush_tile(lu8 tile, uint32_t phase, uint8_t* dst, uint32_t n, uint32_t lane) {
  wave_phase();
  const gu8 g = reinterpret_cast<gu8>(reinterpret_cast<uint64_t>(dst));
  const lu8 src = tile + phase;
  uint32_t head = (16u - phase) & 15u;
  head = head < n ? head : n;
  const uint32_t body = (n - head) & ~15u;
  if (lane < head) g[lane] = src[lane];
  for (uint32_t o = head + 16u * lane; o < head + body; o += 1024u)
    *reinterpret_cast<gu32x4>(g + o) = *reinterpret_cast<lcu32x4>(src + o);
  const uint32_t tail = head + body;
  if (tail + lane < n) g[tail + lane] = src[tail + lane];
  wave_phase();
}

struct Ent {
  uint64_t ka, voff, vlen;  // key start; value slice
  uint64_t klen, shared;
  uint64_t size;            // encoded: header + key delta + value
  uint32_t hdr;
  bool bad;
};

// entry j as position k of its block
__device__ __forceinline__ Ent size_entry(const BuildEntries& e, uint64_t j, uint64_t k, uint32_t interval) {
  Ent en = {};
  en.bad = !key_of(e, j, en.ka, en.klen);
  en.voff = e.values[2 * j];
  en.vlen = e.values[2 * j + 1];
  en.bad |= en.voff > e.value_image_size || en.vlen > e.value_image_size - en.voff;
  if (en.bad) return en;
  if (k % interval != 0) {  // (k >= 1: the predecessor is an entry of this block)
    uint64_t pa, plen;
    if (!key_of(e, j - 1, pa, plen)) {
      en.bad = true;
      return en;
    }
    en.shared = common_prefix(gptr(e.keys, pa), plen, gptr(e.keys, en.ka), en.klen);
  }
  en.hdr = varint_len(en.shared) + varint_len(en.klen - en.shared) + varint_len(en.vlen);
  en.size = en.hdr + (en.klen - en.shared) + en.vlen;
  return en;
}

// Up to 64 entries of a block, lane l owning entry l (m of them; off: where
// the lane's entry starts; k: its position in the block).
template <class P>
__device__ __forceinline__ void write_entries(P d, const BuildEntries& e, const Ent& en, uint64_t off, uint64_t k,
                                              uint32_t m, uint32_t interval, uint64_t restarts_at, uint32_t lane) {
  if (lane < m) {
    uint64_t p = put_varint(d, off, en.shared);
    p = put_varint(d, p, en.klen - en.shared);
    put_varint(d, p, en.vlen);
    if (k % interval == 0) put_le32(d, restarts_at + 4 * (k / interval), (uint32_t)off);
  }
  for (uint32_t q = 0; q < m; q++) {
    const uint64_t ns = bcast64(en.klen - en.shared, q), n = ns + bcast64(en.vlen, q);
    const gcu8 key = gptr(e.keys, bcast64(en.ka + en.shared, q));
    const gcu8 val = gptr(e.value_image, bcast64(en.voff, q));
    const uint64_t at = bcast64(off, q) + bcast32(en.hdr, q);
    for (uint64_t i = lane; i < n; i += 64) d[at + i] = i < ns ? key[i] : val[i - ns];
  }
}

template <class P>
__device__ __forceinline__ void write_block(P d, const BuildArgs& a, uint64_t e0, uint64_t n, const Ent& first, uint64_t fin,
                                            uint32_t lane) {
  const uint64_t ri = a.restart_interval;
  const uint64_t nr = n ? (n + ri - 1) / ri : 1, restarts_at = fin - 4 - 4 * nr;
  uint64_t carry = 0;
  for (uint64_t c = 0; c < n; c += 64) {
    const uint32_t m = n - c < 64 ? (uint32_t)(n - c) : 64u;
    Ent en = first;
    if (c != 0) {
      en = Ent{};
      if (lane < m) en = size_entry(a.e, e0 + c + lane, c + lane, a.restart_interval);
    }
    const uint64_t inc = wave_incl_scan(lane < m ? en.size : 0, lane);
    write_entries(d, a.e, en, carry + inc - en.size, c + lane, m, a.restart_interval, restarts_at, lane);
    carry += bcast64(inc, 63);
  }
  if (lane == 0) {
    if (n == 0) put_le32(d, 0, 0);  // Finish() of a fresh builder: restarts_ = {0}
    put_le32(d, fin - 4, (uint32_t)nr);
  }
}

__global__ __launch_bounds__(kBuildThreads) void block_build_kernel(BuildArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tiles[kBuildWaves][kBuildTileAlloc];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const lu8 tile = (lu8)tiles[wv];
  const uint64_t stride = (uint64_t)gridDim.x * kBuildWaves;
  for (uint64_t b = (uint64_t)blockIdx.x * kBuildWaves + wv; b < a.n_blocks; b += stride) {
    const uint64_t e0 = a.block_first[b], e1 = a.block_first[b + 1];
    const uint64_t w_off = a.out_handles[2 * b], w_size = a.out_handles[2 * b + 1];
    uint32_t status = kBuildOk;
    uint64_t fin = 0;
    Ent first = {};
    if (e0 > e1 || e1 > a.e.n || w_off > a.out_size || w_size > a.out_size - w_off) {
      status = kBuildBadInput;
    } else {
      // pass 1: every entry's bounds, and the block's size
      const uint64_t n = e1 - e0, ri = a.restart_interval;
      uint64_t tot = 0;
      for (uint64_t c = 0; c < n && status == kBuildOk; c += 64) {
        Ent en = {};
        if (c + lane < n) en = size_entry(a.e, e0 + c + lane, c + lane, a.restart_interval);
        if (c == 0) first = en;
        if (__ballot(en.bad) != 0ull) status = kBuildBadInput;
        // (an entry is at most 15 + keys_size + value_image_size bytes: 64 of them do not wrap)
        tot += wave_sum(en.bad ? 0 : en.size);
        if (tot >= kMaxBlock) status = status > kBuildTooLarge ? status : kBuildTooLarge;
      }
      fin = tot + 4 * (n ? (n + ri - 1) / ri : 1) + 4;
      if (status == kBuildOk && fin >= kMaxBlock) status = kBuildTooLarge;
      if (status != kBuildOk) {
        fin = 0;
      } else if (fin > w_size) {
        status = kBuildNoRoom;
      } else if (fin <= kBuildTileBytes) {
        uint8_t* dst = a.out + w_off;
        const uint32_t phase = (uint32_t)(reinterpret_cast<uint64_t>(dst) & 15u);
        write_block(tile + phase, a, e0, n, first, fin, lane);
        flush_tile(tile, phase, dst, (uint32_t)fin, lane);
      } else {
        write_block(gwptr(a.out, w_off), a, e0, n, first, fin, lane);
      }
    }
    if (lane == 0) {
      a.status[b] = status;
      if (a.built_bytes) a.built_bytes[b] = fin;
    }
  }
}

// ---------------------------------------------------------------- index block

// An index key: key[src, src + copy), then (bump) the byte key[src + copy] + 1,
// then (tag) kMaxSequenceNumber << 8 | kValueTypeForSeek as a fixed64.
struct IdxEnt {
  uint64_t src, copy;
  uint64_t h_off, h_size;
  uint64_t klen, size;
  uint32_t vlen;
  bool bump, tag, bad;
};

__device__ __forceinline__ IdxEnt index_entry(const IndexArgs& a, uint64_t b, bool last_of_table) {
  IdxEnt x = {};
  x.bad = true;
  const uint64_t f0 = a.block_first[b], f1 = a.block_first[b + 1];
  if (f0 >= f1 || f1 > a.e.n) return x;  // (a block without entries has no last key)
  uint64_t sa, slen, la = 0, llen = 0;
  if (!key_of(a.e, f1 - 1, sa, slen)) return x;
  if (!last_of_table && (f1 >= a.e.n || !key_of(a.e, f1, la, llen))) return x;
  const uint64_t strip = a.cmp == 1 ? 8 : 0;  // LSBM_CMP_INTERNAL_KEY: ExtractUserKey
  if (slen < strip || (!last_of_table && llen < strip)) return x;
  const uint64_t us = slen - strip;
  const gcu8 s = gptr(a.e.keys, sa);
  uint64_t d;
  bool changed = false;
  if (last_of_table) {  // FindShortSuccessor: the first byte that can be incremented
    d = 0;
    while (d < us && s[d] == 0xffu) d++;
    changed = d < us;
  } else {              // FindShortestSeparator
    const gcu8 l = gptr(a.e.keys, la);
    const uint64_t ul = llen - strip, m = us < ul ? us : ul;
    d = common_prefix(s, us, l, ul);
    changed = d < m && s[d] != 0xffu && (uint32_t)s[d] + 1u < (uint32_t)l[d];
  }
  // (the internal comparator keeps the key unless its user part got shorter)
  if (changed && strip && d + 1 >= us) changed = false;
  x.bad = false;
  x.src = sa;
  x.copy = changed ? d : slen;
  x.bump = changed;
  x.tag = changed && strip;
  x.h_off = a.data_handles[2 * b];
  x.h_size = a.data_handles[2 * b + 1];
  x.klen = x.copy + (x.bump ? 1 : 0) + (x.tag ? 8 : 0);
  x.vlen = varint_len(x.h_off) + varint_len(x.h_size);
  x.size = 1 + varint_len(x.klen) + 1 + x.klen + x.vlen;  // shared = 0; a handle is at most 20 bytes
  return x;
}

template <class P>
__device__ __forceinline__ void write_index_entry(P d, const IndexArgs& a, const IdxEnt& x, uint64_t off) {
  d[off] = 0;
  uint64_t p = put_varint(d, off + 1, x.klen);
  d[p++] = (uint8_t)x.vlen;
  const gcu8 s = gptr(a.e.keys, x.src);
  for (uint64_t i = 0; i < x.copy; i++) d[p + i] = s[i];
  p += x.copy;
  if (x.bump) d[p++] = (uint8_t)(s[x.copy] + 1u);
  if (x.tag) {
    d[p++] = 1;  // kValueTypeForSeek
    for (int i = 0; i < 7; i++) d[p++] = 0xffu;
  }
  p = put_varint(d, p, x.h_off);
  put_varint(d, p, x.h_size);
}

template <class P>
__device__ __forceinline__ void write_index(P d, const IndexArgs& a, uint64_t b0, uint64_t n, const IdxEnt& first, uint64_t fin,
                                            uint32_t lane) {
  const uint64_t nr = n ? n : 1, restarts_at = fin - 4 - 4 * nr;
  uint64_t carry = 0;
  for (uint64_t c = 0; c < n; c += 64) {
    const bool mine = c + lane < n;
    IdxEnt x = first;
    if (c != 0) {
      x = IdxEnt{};
      if (mine) x = index_entry(a, b0 + c + lane, c + lane + 1 == n);
    }
    const uint64_t inc = wave_incl_scan(mine ? x.size : 0, lane);
    if (mine) {
      const uint64_t off = carry + inc - x.size;
      write_index_entry(d, a, x, off);
      put_le32(d, restarts_at + 4 * (c + lane), (uint32_t)off);
    }
    carry += bcast64(inc, 63);
  }
  if (lane == 0) {
    if (n == 0) put_le32(d, 0, 0);
    put_le32(d, fin - 4, (uint32_t)nr);
  }
}

__global__ __launch_bounds__(kBuildThreads) void index_build_kernel(IndexArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tiles[kBuildWaves][kBuildTileAlloc];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const lu8 tile = (lu8)tiles[wv];
  const uint64_t stride = (uint64_t)gridDim.x * kBuildWaves;
  for (uint64_t t = (uint64_t)blockIdx.x * kBuildWaves + wv; t < a.n_tables; t += stride) {
    const uint64_t b0 = a.table_block_first[t], b1 = a.table_block_first[t + 1];
    uint32_t status = kBuildOk;
    uint64_t fin = 0, w_off = 0, w_size = 0;
    if (a.out) {
      w_off = a.out_handles[2 * t];
      w_size = a.out_handles[2 * t + 1];
    }
    IdxEnt first = {};
    if (b0 > b1 || b1 > a.n_blocks || w_off > a.out_size || w_size > a.out_size - w_off) {
      status = kBuildBadInput;
    } else {
      const uint64_t n = b1 - b0;
      uint64_t tot = 0;
      for (uint64_t c = 0; c < n && status == kBuildOk; c += 64) {
        IdxEnt x = {};
        if (c + lane < n) x = index_entry(a, b0 + c + lane, c + lane + 1 == n);
        if (c == 0) first = x;
        if (__ballot(x.bad) != 0ull) status = kBuildBadInput;
        tot += wave_sum(x.bad ? 0 : x.size);
        if (tot >= kMaxBlock) status = status > kBuildTooLarge ? status : kBuildTooLarge;
      }
      fin = tot + 4 * (n ? n : 1) + 4;
      if (status == kBuildOk && fin >= kMaxBlock) status = kBuildTooLarge;
      if (status != kBuildOk) {
        fin = 0;
      } else if (!a.out) {
        // sizes only
      } else if (fin > w_size) {
        status = kBuildNoRoom;
      } else if (fin <= kBuildTileBytes) {
        uint8_t* dst = a.out + w_off;
        const uint32_t phase = (uint32_t)(reinterpret_cast<uint64_t>(dst) & 15u);
        write_index(tile + phase, a, b0, n, first, fin, lane);
        flush_tile(tile, phase, dst, (uint32_t)fin, lane);
      } else {
        write_index(gwptr(a.out, w_off), a, b0, n, first, fin, lane);
      }
    }
    if (lane == 0) {
      a.status[t] = status;
      a.built_bytes[t] = fin;
    }
  }
}

}  // namespace

hipError_t launch_block_plan(const PlanArgs& a, int entry_grid, int table_wave_grid, int table_grid, hipStream_t stream) {
  if (a.e.n) {
    hipLaunchKernelGGL(plan_sizes_kernel, dim3(entry_grid), dim3(kBuildThreads), 0, stream, a);
    hipLaunchKernelGGL(plan_links_kernel, dim3(entry_grid), dim3(kBuildThreads), 0, stream, a);
  }
  if (a.n_tables) hipLaunchKernelGGL(plan_chain_kernel, dim3(table_wave_grid), dim3(kBuildThreads), 0, stream, a);
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(64), 0, stream, a);
  if (a.n_tables) hipLaunchKernelGGL(plan_emit_kernel, dim3(table_grid), dim3(kBuildThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_block_build(const BuildArgs& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(block_build_kernel, dim3(grid), dim3(kBuildThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_index_build(const IndexArgs& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(index_build_kernel, dim3(grid), dim3(kBuildThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
