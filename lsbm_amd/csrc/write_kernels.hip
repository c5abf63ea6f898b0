// write_kernels.hip -- gfx950 kernels of the batched DB::Write
// (include/lsbm_write.h): WriteBatch::Put / Delete's encoding, DBImpl::
// BuildBatchGroup's rule, WriteBatchInternal::Append / SetSequence / SetCount,
// and log::Writer::AddRecord's framing with the CRC bytes left zero.
//
// sizes   wr_size_tile     one lane per op: its encoded size, checked; a sum per tile
//         wr_scan_tiles    one workgroup: the tiles' running sums
//         wr_size_apply    one lane per op: op_sum
//         wr_batch_sum     one lane per writer: 12 w + op_sum[batch_first[w]]
// group   wr_next_sync     one workgroup: the first sync writer after each writer
//         wr_group_links   one lane per writer: "if a group started here, where
//                          would it end" -- a binary search in the running sums
//         wr_group_chain   one wave: lane 0 hops through the links, staged in
//                          LDS kWrChainChunk at a time
//         wr_group_emit    group_first / group_sync, dense
// build   wr_build_check   every op, writer and group against the sums
//         wr_build_plan    one lane per group: records, sequence, count
//         wr_build_move    one lane per 16 destination bytes of the rep image
// frame   wr_frame_check   one lane per record: its slice against the image
//         wr_frame_plan    one wave: AddRecord's arithmetic, 64 records a step
//                          between events, lengths staged in LDS
//         wr_frame_verify  one lane per record: the plan, link by link
//         wr_frame_move    one lane per 16 destination bytes of the window,
//                          then one lane per record for its header offsets
//
// The movers are destination-centric: a lane owns one 16-byte aligned chunk of
// the output, finds the op or record its first byte belongs to by binary
// search, and either copies 16 source bytes (two 8-byte loads at any
// alignment, one aligned 16-byte store) where the chunk lies inside one key,
// value or payload fragment, or assembles the chunk byte by byte in registers
// across headers, varints and neighbours.  Only the first and the last chunk
// of an output leave as single bytes.
//
// Every call has one status word.  It is zeroed by the engine, raised by the
// check kernels, and every kernel that writes an output leaves at once when it
// is set: on an error no other output changes.  Every offset and length of
// the input is untrusted, and so are op_sum, group_first, frag_first and
// rec_start where a later step takes them back in: they are verified link by
// link (each op's size against its slot, each record's end against the next
// start) before a byte is written.  No spin-waits, no cross-workgroup state
// inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // gcu8, gu8, u32x4, gu32x4, gptr, gwptr, load8, wave_phase, block_excl_sum
#include "write_types.h"

namespace lsbm {
namespace {

__device__ __forceinline__ uint32_t varint_len(uint64_t v) {  // util/coding.cc:VarintLength
  uint32_t n = 1;
  while (v >= 128) {
    v >>= 7;
    n++;
  }
  return n;
}

// byte t of PutVarint32(v)
__device__ __forceinline__ uint32_t varint_byte(uint64_t v, uint32_t t) {
  const uint64_t x = v >> (7 * t);
  return (uint32_t)(x & 127u) | (x >= 128 ? 128u : 0u);
}

__device__ __forceinline__ void wr_raise(uint32_t* status, uint32_t code) { atomicMax(status, code); }

// One op as WriteBatch::Put / Delete appends it (common/write_batch.cc:98-109):
// [0] type, [1, e1) varint klen, [e1, e2) key, [e2, e3) varint vlen, [e3, size) value.
struct Op {
  uint64_t koff, klen, voff, vlen, size;
  uint32_t type, e1;
  bool bad;
  __device__ __forceinline__ uint64_t e2() const { return e1 + klen; }
};

__device__ __forceinline__ Op op_of(const WrOps& o, uint64_t j) {
  Op d = {};
  d.type = o.types[j];
  const uint64_t a = o.key_offsets[j], b = o.key_offsets[j + 1];
  d.koff = a;
  d.klen = b - a;
  d.bad = d.type > 1u || a > b || b > o.keys_size || (d.klen >> 32) != 0;
  if (d.type == 1u) {
    d.voff = o.values[2 * j];
    d.vlen = o.values[2 * j + 1];
    d.bad |= (d.vlen >> 32) != 0 || d.voff > o.value_image_size || d.vlen > o.value_image_size - d.voff;
  }
  if (d.bad) return d;
  d.e1 = 1 + varint_len(d.klen);
  d.size = (uint64_t)d.e1 + d.klen + (d.type ? varint_len(d.vlen) + d.vlen : 0);
  return d;
}
// where the value starts (a Delete has none: vlen is 0 and this is the op's size)
__device__ __forceinline__ uint64_t e3_of(const Op& d) { return d.size - d.vlen; }

// batch_first is monotone from 0 to n_ops
__device__ __forceinline__ void check_batches(const WrOps& o, uint32_t* status, uint64_t first, uint64_t stride) {
  for (uint64_t w = first; w < o.n_writers; w += stride) {
    const uint64_t a = o.batch_first[w], b = o.batch_first[w + 1];
    if (a > b || b > o.n) wr_raise(status, kWrBadInput);
  }
  if (first == 0 && (o.batch_first[0] != 0 || o.batch_first[o.n_writers] != o.n)) wr_raise(status, kWrBadInput);
}

// ---------------------------------------------------------------- sizes

__global__ __launch_bounds__(kWrThreads) void wr_size_tile_kernel(WrSizesArgs a) {
  __shared__ uint64_t row[kWrWaves];
  if (blockIdx.x < a.n_tiles) {
    const uint64_t j = global_index<kWrThreads>();
    uint64_t size = 0;
    if (j < a.o.n) {
      const Op d = op_of(a.o, j);
      if (d.bad) wr_raise(a.status, kWrBadInput);
      size = d.size;
    }
    uint64_t excl, total;
    block_excl_sum<kWrWaves>(size, row, excl, total);
    if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
  }
  check_batches(a.o, a.status, global_index<kWrThreads>(), (uint64_t)gridDim.x * kWrThreads);
}

// tiles[0, n_tiles) -> their exclusive running sums in place, the total in tiles[n_tiles]
__global__ __launch_bounds__(kWrThreads) void wr_scan_tiles_kernel(WrSizesArgs a) {
  __shared__ uint64_t row[kWrWaves];
  uint64_t carry = 0;
  for (uint64_t c = 0; c < a.n_tiles; c += kWrThreads) {
    const uint64_t t = c + threadIdx.x, v = t < a.n_tiles ? a.tiles[t] : 0;
    uint64_t excl, total;
    block_excl_sum<kWrWaves>(v, row, excl, total);
    if (t < a.n_tiles) a.tiles[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.tiles[a.n_tiles] = carry;
    if (*a.status == kWrOk) a.op_sum[a.o.n] = carry;
  }
}

__global__ __launch_bounds__(kWrThreads) void wr_size_apply_kernel(WrSizesArgs a) {
  __shared__ uint64_t row[kWrWaves];
  if (*a.status != kWrOk) return;
  const uint64_t j = global_index<kWrThreads>();
  const uint64_t size = j < a.o.n ? op_of(a.o, j).size : 0;
  uint64_t excl, total;
  block_excl_sum<kWrWaves>(size, row, excl, total);
  if (j < a.o.n) a.op_sum[j] = a.tiles[blockIdx.x] + excl;
}

// WriteBatchInternal::ByteSize, summed: batch w's rep is 12 bytes and its ops
__global__ __launch_bounds__(kWrThreads) void wr_batch_sum_kernel(WrSizesArgs a) {
  if (*a.status != kWrOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t w = global_index<kWrThreads>(); w <= a.o.n_writers; w += stride)
    a.batch_sum[w] = 12 * w + a.op_sum[a.o.batch_first[w]];
}

// ---------------------------------------------------------------- group rule

// nsync[w]: the smallest w' > w with sync[w'], or n.  One workgroup walks the
// writers from the end, a tile at a time, carrying the minimum so far.
__global__ __launch_bounds__(kWrThreads) void wr_next_sync_kernel(WrGroupArgs a) {
  __shared__ uint32_t row[kWrWaves];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, n = (uint32_t)a.n;
  uint32_t carry = n;
  for (uint64_t c = (a.n + kWrThreads - 1) / kWrThreads; c-- > 0;) {
    const uint64_t w = c * kWrThreads + threadIdx.x;
    const uint32_t v = (w < a.n && a.sync[w]) ? (uint32_t)w : n;
    uint32_t incl = v;  // the minimum over this lane and the wave's later lanes
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_down((int)incl, o);
      if (lane + o < 64 && t < incl) incl = t;
    }
    const uint32_t next = (uint32_t)__shfl_down((int)incl, 1);
    if (lane == 0) row[wv] = incl;
    __syncthreads();
    uint32_t after = carry, all = carry;
    for (uint32_t i = 0; i < kWrWaves; i++) {
      const uint32_t t = row[i];
      if (i > wv && t < after) after = t;
      if (t < all) all = t;
    }
    if (lane < 63 && next < after) after = next;
    if (w < a.n) a.nsync[w] = after;
    carry = all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWrThreads) void wr_group_links_kernel(WrGroupArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t f = global_index<kWrThreads>(); f < a.n; f += stride) {
    const uint64_t s0 = a.batch_sum[f], s1 = a.batch_sum[f + 1];
    if (s1 < s0 || s1 - s0 < 12) {  // (ByteSize is at least the header; the search below needs the sums to grow)
      wr_raise(a.status, kWrBadInput);
      a.link[f] = 1;
      continue;
    }
    const uint64_t size = s1 - s0, max_size = size <= kGroupSmall ? size + kGroupSmall : kGroupMax;
    // the largest e in [f + 1, n] with batch_sum[e] - batch_sum[f] <= max_size: the leader always counts
    uint64_t lo = f + 1, hi = a.n + 1;
    while (hi - lo > 1) {
      const uint64_t mid = lo + ((hi - lo) >> 1), s = a.batch_sum[mid];
      if (s >= s0 && s - s0 <= max_size) lo = mid; else hi = mid;
    }
    if (a.sync && !a.sync[f]) {  // a sync writer does not join a group led by a non-sync one: checked first
      const uint64_t ns = a.nsync[f];
      lo = ns < lo ? ns : lo;
    }
    a.link[f] = (uint32_t)(lo - f);
  }
}

__global__ __launch_bounds__(64) void wr_group_chain_kernel(WrGroupArgs a) {
  __shared__ uint32_t links[kWrChainChunk];
  if (*a.status != kWrOk) return;
  const uint32_t lane = threadIdx.x;
  uint64_t cur = 0, ng = 0;
  while (cur < a.n) {
    const uint64_t c0 = cur, cn = a.n - c0 < kWrChainChunk ? a.n - c0 : kWrChainChunk;
    for (uint64_t i = lane; i < cn; i += 64) links[i] = a.link[c0 + i];
    wave_phase();
    if (lane == 0) {
      while (cur - c0 < cn) {  // (a link is at least 1)
        a.starts[ng++] = (uint32_t)cur;
        cur += links[cur - c0];
      }
    }
    cur = __shfl(cur, 0);
    ng = __shfl(ng, 0);
    wave_phase();
  }
  if (lane == 0) a.count[0] = ng;
}

__global__ __launch_bounds__(kWrThreads) void wr_group_emit_kernel(WrGroupArgs a) {
  if (*a.status != kWrOk) return;
  const uint64_t ng = a.count[0];
  if (ng > a.groups_cap) {
    if (global_index<kWrThreads>() == 0) wr_raise(a.status, kWrNoRoom);
    return;
  }
  const uint64_t stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t g = global_index<kWrThreads>(); g < ng; g += stride) {
    const uint64_t f = a.starts[g];
    a.group_first[g] = f;
    a.group_sync[g] = (a.sync && a.sync[f]) ? 1 : 0;
  }
  if (global_index<kWrThreads>() == 0) {
    a.group_first[ng] = a.n;
    a.n_groups[0] = ng;
  }
}

// ---------------------------------------------------------------- build

__global__ __launch_bounds__(kWrThreads) void wr_build_check_kernel(WrBuildArgs a) {
  const uint64_t first = global_index<kWrThreads>(), stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t j = first; j < a.o.n; j += stride) {
    const Op d = op_of(a.o, j);
    const uint64_t s0 = a.op_sum[j], s1 = a.op_sum[j + 1];
    if (d.bad || s1 < s0 || s1 - s0 != d.size) wr_raise(a.status, kWrBadInput);
  }
  check_batches(a.o, a.status, first, stride);
  for (uint64_t g = first; g < a.n_groups; g += stride) {
    const uint64_t f0 = a.group_first[g], f1 = a.group_first[g + 1];
    if (f0 >= f1 || f1 > a.o.n_writers) wr_raise(a.status, kWrBadInput);  // (a group has its leader)
  }
  if (first == 0) {
    if (a.op_sum[0] != 0 || a.group_first[0] != 0 || a.group_first[a.n_groups] != a.o.n_writers)
      wr_raise(a.status, kWrBadInput);
    const uint64_t body = a.op_sum[a.o.n];
    if (body > a.reps_cap || 12 * a.n_groups > a.reps_cap - body) wr_raise(a.status, kWrNoRoom);
  }
}

__global__ __launch_bounds__(kWrThreads) void wr_build_plan_kernel(WrBuildArgs a) {
  if (*a.status != kWrOk) return;
  const uint64_t first = global_index<kWrThreads>(), stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t g = first; g < a.n_groups; g += stride) {
    const uint64_t j0 = a.o.batch_first[a.group_first[g]], j1 = a.o.batch_first[a.group_first[g + 1]];
    const uint64_t b0 = a.op_sum[j0];
    a.records[2 * g] = 12 * g + b0;
    a.records[2 * g + 1] = 12 + a.op_sum[j1] - b0;
    a.seq_counts[2 * g] = a.last_sequence + 1 + j0;  // sequence_{g+1} = sequence_g + count_g (db_impl.cc:1342-1343)
    a.seq_counts[2 * g + 1] = j1 - j0;
  }
  if (first == 0) a.new_last_sequence[0] = a.last_sequence + a.o.n;
}

// A chunk's 16 bytes as they are assembled, and how they leave.
struct Chunk {
  uint64_t lo, hi;
  __device__ __forceinline__ void put(uint32_t i, uint32_t byte) {
    if (i < 8) lo |= (uint64_t)byte << (8 * i); else hi |= (uint64_t)byte << (8 * (i - 8));
  }
  __device__ __forceinline__ uint32_t get(uint32_t i) const { return (uint32_t)((i < 8 ? lo : hi) >> (8 * (i & 7))) & 255u; }
  // bytes [i0, i1) of the aligned chunk at address ca
  __device__ __forceinline__ void store(uint64_t ca, uint32_t i0, uint32_t i1) const {
    if (i0 == 0 && i1 == kWrChunk) {
      const u32x4 r = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
      *reinterpret_cast<gu32x4>(ca) = r;
    } else {
      for (uint32_t i = i0; i < i1; i++) *reinterpret_cast<gu8>(ca + i) = (uint8_t)get(i);
    }
  }
};

__global__ __launch_bounds__(kWrThreads) void wr_build_move_kernel(WrBuildArgs a) {
  if (*a.status != kWrOk) return;
  const uint64_t total = 12 * a.n_groups + a.op_sum[a.o.n];
  const uint64_t dst = reinterpret_cast<uint64_t>(a.reps), base = dst & ~(uint64_t)(kWrChunk - 1);
  const uint64_t n_chunks = total ? (dst + total - base + kWrChunk - 1) / kWrChunk : 0;
  const uint64_t stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t c = global_index<kWrThreads>(); c < n_chunks; c += stride) {
    const uint64_t ca = base + c * kWrChunk;
    const uint64_t p0 = ca > dst ? ca - dst : 0, p1 = ca + kWrChunk - dst < total ? ca + kWrChunk - dst : total;
    // the group of the chunk's first byte: the last g with records[2g] <= p0
    uint64_t g = 0, hi = a.n_groups;
    while (hi - g > 1) {
      const uint64_t mid = g + ((hi - g) >> 1);
      if (a.records[2 * mid] <= p0) g = mid; else hi = mid;
    }
    uint64_t r0 = a.records[2 * g], r1 = r0 + a.records[2 * g + 1];  // the group's rep
    uint64_t seq = a.seq_counts[2 * g], cnt = a.seq_counts[2 * g + 1];
    uint64_t j = seq - a.last_sequence - 1;  // its first op; below: the op at hand, [at, at + d.size) in the image
    Op d = {};
    uint64_t at = r0 + 12, end = at;  // (the header stands in for an op that ends where the first one starts)
    bool have = false;
    if (p0 >= r0 + 12) {
      const uint64_t b0 = a.op_sum[j], q = p0 - (r0 + 12) + b0;
      uint64_t lo = j, up = j + cnt;  // the last op with op_sum <= q (an op has 2 bytes or more: no ties)
      while (up - lo > 1) {
        const uint64_t mid = lo + ((up - lo) >> 1);
        if (a.op_sum[mid] <= q) lo = mid; else up = mid;
      }
      j = lo;
      d = op_of(a.o, j);
      at = r0 + 12 + a.op_sum[j] - b0;
      end = at + d.size;
      have = true;
    }
    Chunk k = {0, 0};
    const uint32_t i0 = (uint32_t)(dst + p0 - ca);
    if (have && p1 - p0 == kWrChunk) {  // wholly inside one key or one value: 16 source bytes as they are
      const uint64_t r = p0 - at, e3 = e3_of(d);
      const uint8_t* src = nullptr;
      if (r >= d.e1 && r + kWrChunk <= d.e2()) src = a.o.keys + d.koff + (r - d.e1);
      else if (r >= e3 && r + kWrChunk <= d.size) src = a.o.value_image + d.voff + (r - e3);
      if (src) {
        k.lo = load8(gptr(src, 0));
        k.hi = load8(gptr(src, 8));
        k.store(ca, 0, kWrChunk);
        continue;
      }
    }
    for (uint64_t p = p0; p < p1; p++) {
      while (p >= r1) {  // the next group's rep starts here
        g++;
        r0 = r1;
        r1 = r0 + a.records[2 * g + 1];
        seq = a.seq_counts[2 * g];
        cnt = a.seq_counts[2 * g + 1];
        j = seq - a.last_sequence - 1;
        at = end = r0 + 12;
        have = false;
      }
      uint32_t byte;
      if (p < r0 + 12) {  // fixed64(sequence) || fixed32(count)
        const uint32_t h = (uint32_t)(p - r0);
        byte = h < 8 ? (uint32_t)(seq >> (8 * h)) & 255u : (uint32_t)(cnt >> (8 * (h - 8))) & 255u;
      } else {
        if (p >= end) {  // the next op of the group (p < r1: there is one)
          if (have) j++;
          d = op_of(a.o, j);
          at = end;
          end = at + d.size;
          have = true;
        }
        const uint64_t r = p - at, e2 = d.e2(), e3 = e3_of(d);
        if (r == 0) byte = d.type;
        else if (r < d.e1) byte = varint_byte(d.klen, (uint32_t)r - 1);
        else if (r < e2) byte = a.o.keys[d.koff + (r - d.e1)];
        else if (r < e3) byte = varint_byte(d.vlen, (uint32_t)(r - e2));
        else byte = a.o.value_image[d.voff + (r - e3)];
      }
      k.put(i0 + (uint32_t)(p - p0), byte);
    }
    k.store(ca, i0, i0 + (uint32_t)(p1 - p0));
  }
}

// ---------------------------------------------------------------- frame

// log::Writer::AddRecord (common/log_writer.cc:27-73) of a record of L bytes
// whose first header is at file offset s (s % 32768 <= 32761: a header fits):
// where it ends and how many physical records it is.
__device__ __forceinline__ void frame_step(uint64_t s, uint64_t L, uint64_t& end, uint64_t& frags) {
  const uint64_t b = s & (kLogBlock - 1), a0 = kLogPayload - b;
  if (L <= a0) {
    end = s + kLogHeader + L;
    frags = 1;
  } else {  // FIRST of a0 bytes (0 when exactly 7 are left), k MIDDLE of a whole block, LAST
    const uint64_t rem = L - a0, k = (rem - 1) / kLogPayload;
    end = (s - b) + kLogBlock * (1 + k) + kLogHeader + (rem - k * kLogPayload);
    frags = 2 + k;
  }
}
// where the next record's header goes after a record that ended at file offset e
__device__ __forceinline__ uint64_t frame_pad(uint64_t e) {
  const uint64_t left = kLogBlock - (e & (kLogBlock - 1));
  return left < kLogHeader ? e + left : e;
}
__device__ __forceinline__ bool frame_phase_bad(uint64_t log_offset) {  // no log the reference wrote has this size
  const uint64_t b = log_offset & (kLogBlock - 1);
  return b > 0 && b < kLogHeader;
}

__global__ __launch_bounds__(kWrThreads) void wr_frame_check_kernel(WrFrameArgs a) {
  const uint64_t first = global_index<kWrThreads>(), stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t i = first; i < a.n; i += stride) {
    const uint64_t off = a.records[2 * i], len = a.records[2 * i + 1];
    if (off > a.image_size || len > a.image_size - off) wr_raise(a.status, kWrBadInput);
  }
  if (first == 0 && frame_phase_bad(a.log_offset)) wr_raise(a.status, kWrBadInput);
}

// AddRecord's arithmetic, 64 records a step.  The start of record i + 1 depends
// on record i's, but between *events* the dependence is a plain sum: with
// u = 32761 * block + block offset, a record of L bytes moves u by 7 + L
// whatever it crosses (every later fragment's header is paid for by the 7
// bytes a block holds beyond its 32,761).  An event is a record that ends
// with fewer than 7 bytes left in its block (zero trailer) or exactly on the
// block's end: the next record then starts at block offset 0, which no sum
// arrives at.  So a step takes the known start of its first record, gives
// every lane its start from a prefix sum (u a multiple of 32761 can only be
// block offset 32761 of the block before: exactly 7 bytes left), lets each
// lane run the closed form on its own record, commits through the first
// event found by a ballot, and restarts after it.  Records that all end on a
// block end degrade to one a step.  Lengths are staged in LDS kWrChainChunk
// at a time.
__global__ __launch_bounds__(64) void wr_frame_plan_kernel(WrFrameArgs a) {
  __shared__ uint64_t lens[kWrChainChunk];
  if (*a.status != kWrOk) return;
  const uint32_t lane = threadIdx.x;
  uint64_t pos = a.log_offset, nf = 0;  // where the record before ended; the physical records so far
  for (uint64_t c0 = 0; c0 < a.n; c0 += kWrChainChunk) {
    const uint64_t cn = a.n - c0 < kWrChainChunk ? a.n - c0 : kWrChainChunk;
    for (uint64_t i = lane; i < cn; i += 64) lens[i] = a.records[2 * (c0 + i) + 1];
    wave_phase();
    for (uint64_t i0 = 0; i0 < cn;) {
      const uint32_t m = cn - i0 < 64 ? (uint32_t)(cn - i0) : 64u;
      const bool mine = lane < m;
      const uint64_t s0 = frame_pad(pos), u0 = (s0 / kLogBlock) * kLogPayload + (s0 & (kLogBlock - 1));
      const uint64_t len = mine ? lens[i0 + lane] : 0, cost = mine ? kLogHeader + len : 0;
      const uint64_t u = u0 + wave_incl_scan(cost, lane) - cost;
      uint64_t s = s0;
      if (lane != 0) {
        uint64_t blk = u / kLogPayload, b = u - blk * kLogPayload;
        if (b == 0) {  // (a sum never arrives at a block's start: 7 bytes are left in the block before)
          blk--;
          b = kLogPayload;
        }
        s = blk * kLogBlock + b;
      }
      uint64_t end, frags;
      frame_step(s, len, end, frags);
      const uint64_t eb = end & (kLogBlock - 1);
      const uint64_t events = __ballot(mine && (eb > kLogPayload || eb == 0));
      const uint32_t last = events ? (uint32_t)__builtin_ctzll(events) : m - 1;  // commit through this lane
      const uint64_t fr = lane <= last ? frags : 0, fincl = wave_incl_scan(fr, lane);
      if (lane <= last) {
        a.rec_start[c0 + i0 + lane] = s;
        a.frag_first[c0 + i0 + lane] = nf + fincl - fr;
      }
      pos = __shfl(end, (int)last);
      nf += __shfl(fincl, (int)last);
      i0 += last + 1;
      if (events & 1) {
        // The step's first record was an event, so the step took one record.  Such records come in
        // runs (block-sized ones, each ending on a block end): lane 0 takes the next 64 one by one,
        // which costs a run an LDS read a record instead of a step a record.
        const uint64_t stop = cn - i0 < 64 ? cn : i0 + 64;
        if (lane == 0) {
          for (uint64_t i = i0; i < stop; i++) {
            const uint64_t s1 = frame_pad(pos);
            uint64_t f1;
            frame_step(s1, lens[i], pos, f1);
            a.rec_start[c0 + i] = s1;
            a.frag_first[c0 + i] = nf;
            nf += f1;
          }
        }
        pos = __shfl(pos, 0);
        nf = __shfl(nf, 0);
        i0 = stop;
      }
    }
    wave_phase();
  }
  if (lane == 0) {
    a.rec_start[a.n] = pos;
    a.frag_first[a.n] = nf;
  }
}

// The plan, taken back in: record i starts where record i - 1's end says, and
// is as many fragments as its slots say.  A start past the window is NO_ROOM
// (and, unverified, reads nothing further).
__global__ __launch_bounds__(kWrThreads) void wr_frame_verify_kernel(WrFrameArgs a) {
  const uint64_t first = global_index<kWrThreads>(), stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t i = first; i < a.n; i += stride) {
    const uint64_t s = a.rec_start[i], nxt = a.rec_start[i + 1], len = a.records[2 * i + 1];
    if (s < a.log_offset) {
      wr_raise(a.status, kWrBadInput);
    } else if (s - a.log_offset > a.out_cap) {
      wr_raise(a.status, kWrNoRoom);
    } else {
      uint64_t end, frags;
      frame_step(s, len, end, frags);
      const uint64_t f0 = a.frag_first[i], f1 = a.frag_first[i + 1];
      if ((s & (kLogBlock - 1)) > kLogPayload || nxt != (i + 1 < a.n ? frame_pad(end) : end) || f1 < f0 ||
          f1 - f0 != frags)
        wr_raise(a.status, kWrBadInput);
    }
  }
  if (first == 0) {
    const uint64_t s0 = a.rec_start[0], end = a.rec_start[a.n];
    if (a.frag_first[0] != 0 || s0 != (a.n ? frame_pad(a.log_offset) : a.log_offset) || end < a.log_offset)
      wr_raise(a.status, kWrBadInput);
    else if (end - a.log_offset > a.out_cap || a.frag_first[a.n] > a.headers_cap)
      wr_raise(a.status, kWrNoRoom);
  }
}

// One record of the plan as the mover walks it.
struct Rec {
  uint64_t s, nxt, off, len, blk0, a0;
  __device__ __forceinline__ void load(const WrFrameArgs& a, uint64_t i) {
    s = a.rec_start[i];
    nxt = a.rec_start[i + 1];
    off = a.records[2 * i];
    len = a.records[2 * i + 1];
    blk0 = s / kLogBlock;
    a0 = kLogPayload - (s & (kLogBlock - 1));
  }
  // byte r of fragment t's header, CRC bytes zero (EmitPhysicalRecord, common/log_writer.cc:79-83)
  __device__ __forceinline__ uint32_t header(uint64_t t, uint32_t r) const {
    if (r < 4) return 0;
    const uint64_t left = t == 0 ? len : len - a0 - (t - 1) * kLogPayload, room = t == 0 ? a0 : kLogPayload;
    const bool last = left <= room;
    const uint64_t n = last ? left : room;
    if (r == 4) return (uint32_t)n & 255u;
    if (r == 5) return (uint32_t)(n >> 8);
    return t == 0 ? (last ? 1u : 2u) : (last ? 4u : 3u);  // kFullType, kFirstType, kLastType, kMiddleType
  }
  // file offset f in [s, nxt): the payload index it holds (false: a header byte, in hdr)
  __device__ __forceinline__ bool payload(uint64_t f, uint64_t& pi, uint64_t& pe, uint32_t& hdr) const {
    const uint64_t t = f / kLogBlock - blk0, r = t == 0 ? f - s : (f & (kLogBlock - 1));
    if (r < kLogHeader) {
      hdr = header(t, (uint32_t)r);
      return false;
    }
    pi = (t == 0 ? 0 : a0 + (t - 1) * kLogPayload) + (r - kLogHeader);
    pe = t == 0 ? a0 : a0 + t * kLogPayload;  // the fragment's payload ends here, or where the record does
    pe = pe < len ? pe : len;
    return true;
  }
};

__global__ __launch_bounds__(kWrThreads) void wr_frame_move_kernel(WrFrameArgs a) {
  if (*a.status != kWrOk) return;
  const uint64_t total = a.rec_start[a.n] - a.log_offset;
  const uint64_t dst = reinterpret_cast<uint64_t>(a.out), base = dst & ~(uint64_t)(kWrChunk - 1);
  const uint64_t n_chunks = total ? (dst + total - base + kWrChunk - 1) / kWrChunk : 0;
  const uint64_t first = global_index<kWrThreads>(), stride = (uint64_t)gridDim.x * kWrThreads;
  for (uint64_t c = first; c < n_chunks; c += stride) {
    const uint64_t ca = base + c * kWrChunk;
    const uint64_t p0 = ca > dst ? ca - dst : 0, p1 = ca + kWrChunk - dst < total ? ca + kWrChunk - dst : total;
    const uint64_t f0 = a.log_offset + p0;
    // the record of the chunk's first byte: the last i with rec_start[i] <= f0 (before record 0: the leading pad)
    uint64_t i = 0, hi = a.n;
    while (hi - i > 1) {
      const uint64_t mid = i + ((hi - i) >> 1);
      if (a.rec_start[mid] <= f0) i = mid; else hi = mid;
    }
    Rec rc;
    rc.load(a, i);
    Chunk k = {0, 0};
    const uint32_t i0 = (uint32_t)(dst + p0 - ca);
    uint64_t pi, pe;
    uint32_t hdr;
    if (p1 - p0 == kWrChunk && f0 >= rc.s && rc.payload(f0, pi, pe, hdr) && pi + kWrChunk <= pe) {
      const uint8_t* src = a.image + rc.off + pi;  // wholly inside one fragment's payload
      k.lo = load8(gptr(src, 0));
      k.hi = load8(gptr(src, 8));
      k.store(ca, 0, kWrChunk);
      continue;
    }
    for (uint64_t p = p0; p < p1; p++) {
      const uint64_t f = a.log_offset + p;
      while (f >= rc.nxt) rc.load(a, ++i);  // (f < the end: there is a next record)
      uint32_t byte = 0;  // the leading pad, and a block's trailer after a record's end
      if (f >= rc.s) {
        if (!rc.payload(f, pi, pe, hdr)) byte = hdr;
        else if (pi < pe) byte = a.image[rc.off + pi];
      }
      k.put(i0 + (uint32_t)(p - p0), byte);
    }
    k.store(ca, i0, i0 + (uint32_t)(p1 - p0));
  }
  // the headers, window-relative, in file order
  for (uint64_t r = first; r < a.n; r += stride) {
    const uint64_t s = a.rec_start[r], h0 = a.frag_first[r], nf = a.frag_first[r + 1] - h0;
    a.headers[h0] = s - a.log_offset;
    const uint64_t blk = s & ~(kLogBlock - 1);
    for (uint64_t t = 1; t < nf; t++) a.headers[h0 + t] = blk + t * kLogBlock - a.log_offset;
  }
}

}  // namespace

hipError_t launch_write_sizes(const WrSizesArgs& a, int writer_grid, hipStream_t stream) {
  const dim3 tiles((uint32_t)(a.n_tiles ? a.n_tiles : 1)), block(kWrThreads);
  hipLaunchKernelGGL(wr_size_tile_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(wr_scan_tiles_kernel, dim3(1), block, 0, stream, a);
  if (a.n_tiles) hipLaunchKernelGGL(wr_size_apply_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(wr_batch_sum_kernel, dim3(writer_grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_write_group(const WrGroupArgs& a, int writer_grid, hipStream_t stream) {
  const dim3 block(kWrThreads);
  if (a.n) {
    if (a.sync) hipLaunchKernelGGL(wr_next_sync_kernel, dim3(1), block, 0, stream, a);
    hipLaunchKernelGGL(wr_group_links_kernel, dim3(writer_grid), block, 0, stream, a);
  }
  hipLaunchKernelGGL(wr_group_chain_kernel, dim3(1), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(wr_group_emit_kernel, dim3(writer_grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_write_build(const WrBuildArgs& a, int check_grid, int group_grid, int move_grid, hipStream_t stream) {
  const dim3 block(kWrThreads);
  hipLaunchKernelGGL(wr_build_check_kernel, dim3(check_grid), block, 0, stream, a);
  hipLaunchKernelGGL(wr_build_plan_kernel, dim3(group_grid), block, 0, stream, a);
  if (a.n_groups) hipLaunchKernelGGL(wr_build_move_kernel, dim3(move_grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_frame_plan(const WrFrameArgs& a, int record_grid, hipStream_t stream) {
  hipLaunchKernelGGL(wr_frame_check_kernel, dim3(record_grid), dim3(kWrThreads), 0, stream, a);
  hipLaunchKernelGGL(wr_frame_plan_kernel, dim3(1), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_frame(const WrFrameArgs& a, int record_grid, int move_grid, hipStream_t stream) {
  const dim3 block(kWrThreads);
  hipLaunchKernelGGL(wr_frame_check_kernel, dim3(record_grid), block, 0, stream, a);
  hipLaunchKernelGGL(wr_frame_verify_kernel, dim3(record_grid), block, 0, stream, a);
  if (a.n) hipLaunchKernelGGL(wr_frame_move_kernel, dim3(move_grid), block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
