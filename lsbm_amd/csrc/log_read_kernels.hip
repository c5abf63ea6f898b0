// log_read_kernels.hip -- gfx950 kernels of the batched log::Reader
// (include/lsbm_log_read.h): ReadPhysicalRecord's block walk, ReadRecord's
// in_fragmented_record / scratch state machine with every Reporter call, and
// the assembly of fragmented records, for a whole log image in one launch
// sequence.
//
// walk    lr_walk_count    one workgroup per 32 KiB block: the block staged in
//                          LDS by 16-byte loads, one lane hops from header to
//                          header in LDS; the block's header count and end
//         lr_walk_scan     one workgroup: the blocks' running header counts
//         lr_walk_list     the same walk, the header offsets written out
//         lr_walk_publish  block_first, block_end, the header count
// plan    lr_plan_check    every header and every block's end against the
//                          image: the walk is verified, not trusted
//         lr_plan_cut      one lane per header: the block's first failed CRC
//         lr_plan_classify one lane per slot (a header, a block's end, the
//                          end of the file): what it is to ReadRecord
//         lr_plan_scan_a   one workgroup: the tiles' last setter and MIDDLE sums
//         lr_plan_state    one lane per slot: the nearest earlier slot that
//                          sets in_fragmented_record outright, the MIDDLE
//                          lengths before it
//         lr_plan_scratch  one lane per slot: in_fragmented_record and
//                          scratch->size() on arrival; a LAST marks its FIRST
//         lr_plan_count    one lane per slot: records, reports, fragments and
//                          side bytes it yields; a sum per tile
//         lr_plan_scan_b   one workgroup: the tiles' running sums, the totals
// emit    lr_emit_check    the caps against the totals
//         lr_emit_slots    one lane per slot: records, last_record_offset,
//                          events; its place in the side area and fragment table
//         lr_emit_frags    one lane per slot: the fragment table
//         lr_emit_move     one lane per 16 destination bytes of the side area
//
// ReadRecord's loop is serial in the reference, but its state on arrival at a
// slot is decided by the nearest earlier slot that sets it outright (FULL,
// LAST, a bad record, an unknown type: not in a fragmented record; FIRST: in
// one, scratch = its length) plus the lengths of the MIDDLEs since, which are
// a running maximum and a running sum.  The stop (type 5, the end of the
// file) is a minimum over slots.  Nothing at or after a block's first failed
// CRC is a slot of its own, nothing after the stop yields anything.
//
// Every call has one status word, zeroed by the engine and raised by the
// check kernels; a kernel that writes an output leaves at once when it is
// set.  No spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // gcu8, gu8, u32x4, gcu32x4, gu32x4, gptr, load8, global_index, block_excl_sum
#include "log_read_types.h"

namespace lsbm {
namespace {

__device__ __forceinline__ void lr_raise(uint32_t* status, uint32_t code) { atomicMax(status, code); }

__device__ __forceinline__ uint64_t block_bytes(uint64_t log_bytes, uint64_t start) {
  return log_bytes - start < kLrBlock ? log_bytes - start : kLrBlock;
}

// how a block's walk ends with `rem` bytes left at a header {len, type} (read only when rem >= 7)
__device__ __forceinline__ uint64_t end_of_walk(uint64_t rem, uint64_t size, uint32_t len, uint32_t t, bool& more) {
  more = false;
  if (rem < kLrHeader) return rem == 0 ? kEndRanOut : (size == kLrBlock ? kEndTrailer : kEndTruncated);
  if (kLrHeader + len > rem) return kEndBadLength;
  if (t == 0 && len == 0) return kEndZeroHeader;
  more = true;
  return kEndRanOut;
}

// ---------------------------------------------------------------- walk

// The dependent chain of a block's walk is one LDS read a record (three byte
// loads issued together), not one HBM round trip.  The block lies in LDS at
// the phase of its global address, so that every staged chunk is an aligned
// 16-byte load and an aligned 16-byte LDS store; the first and the last chunk
// arrive as single bytes and nothing outside the log is read.
template <bool kList>
__global__ __launch_bounds__(kLrThreads) void lr_walk_kernel(LrWalkArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t blk[kLrBlock + 16];
  if (kList && *a.status != kLrOk) return;
  for (uint64_t r = blockIdx.x; r < a.n_blocks; r += gridDim.x) {
    const uint64_t start = (a.first_block + r) * kLrBlock;
    const uint32_t size = (uint32_t)block_bytes(a.log_bytes, start);
    const uint64_t src = reinterpret_cast<uint64_t>(a.image) + a.log_at + start;
    const uint32_t phase = (uint32_t)(src & 15u), stop = phase + size;
    const uint64_t base = src - phase;
    for (uint32_t lo = threadIdx.x * 16u; lo < stop; lo += kLrThreads * 16u) {
      if (lo >= phase && lo + 16 <= stop) {
        *reinterpret_cast<u32x4*>(blk + lo) = *reinterpret_cast<gcu32x4>(base + lo);
      } else {
        const uint32_t i1 = lo + 16 < stop ? lo + 16 : stop;
        for (uint32_t i = lo > phase ? lo : phase; i < i1; i++) blk[i] = *reinterpret_cast<gcu8>(base + i);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint64_t first = kList ? a.counts[r] : 0;
      uint32_t pos = 0, n = 0;
      uint64_t how;
      for (;;) {
        const uint32_t rem = size - pos;
        uint32_t len = 0, t = 0;
        if (rem >= kLrHeader) {
          const uint8_t* h = blk + phase + pos;
          len = h[4] | (uint32_t)h[5] << 8;
          t = h[6];
        }
        bool more;
        how = end_of_walk(rem, size, len, t, more);
        if (!more) break;
        if (kList) a.headers[first + n] = start + pos;
        n++;
        pos += (uint32_t)kLrHeader + len;
      }
      if (!kList) {
        a.counts[r] = n;
        a.ends[2 * r] = how;
        a.ends[2 * r + 1] = size - pos;
      }
    }
    __syncthreads();
  }
}

// counts[0, n_blocks) -> their exclusive running sums in place, the total in counts[n_blocks]
__global__ __launch_bounds__(kLrThreads) void lr_walk_scan_kernel(LrWalkArgs a) {
  __shared__ uint64_t row[kLrWaves];
  uint64_t carry = 0;
  for (uint64_t c = 0; c < a.n_blocks; c += kLrThreads) {
    const uint64_t r = c + threadIdx.x, v = r < a.n_blocks ? a.counts[r] : 0;
    uint64_t excl, total;
    block_excl_sum<kLrWaves>(v, row, excl, total);
    if (r < a.n_blocks) a.counts[r] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.counts[a.n_blocks] = carry;
    if (a.headers && carry > a.headers_cap) lr_raise(a.status, kLrNoRoom);
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_walk_publish_kernel(LrWalkArgs a) {
  if (*a.status != kLrOk) return;
  const uint64_t first = global_index<kLrThreads>(), stride = (uint64_t)gridDim.x * kLrThreads;
  for (uint64_t r = first; r <= a.n_blocks; r += stride) {
    a.block_first[r] = a.counts[r];
    if (r < a.n_blocks) {
      a.block_end[2 * r] = a.ends[2 * r];
      a.block_end[2 * r + 1] = a.ends[2 * r + 1];
    }
  }
  if (first == 0) a.n_headers[0] = a.counts[a.n_blocks];
}

// ---------------------------------------------------------------- plan

__device__ __forceinline__ void header_of(const LrPlan& p, uint64_t o, uint32_t& len, uint32_t& t) {
  gcu8 h = gptr(p.image, p.log_at + o);
  len = h[4] | (uint32_t)h[5] << 8;
  t = h[6];
}

// The walk's arrays taken back in.  A header is listed iff the walk from its
// block's start arrives at it: the block's first header is at the block's
// start, each next one where the one before ends, each fits and is no zero
// header, and what follows the last one is the end the walk gave.
__global__ __launch_bounds__(kLrThreads) void lr_plan_check_kernel(LrPlan p) {
  const uint64_t first = global_index<kLrThreads>(), stride = (uint64_t)gridDim.x * kLrThreads;
  for (uint64_t k = first; k < p.n_headers; k += stride) {
    const uint64_t o = p.headers[k], b = o / kLrBlock;
    bool bad = o >= p.log_bytes || p.log_bytes - o < kLrHeader || b < p.first_block || b - p.first_block >= p.n_blocks;
    if (!bad) {
      const uint64_t r = b - p.first_block, f0 = p.block_first[r], f1 = p.block_first[r + 1];
      const uint64_t start = b * kLrBlock, rem = start + block_bytes(p.log_bytes, start) - o;
      uint32_t len, t;
      header_of(p, o, len, t);
      bad = k < f0 || k >= f1 || kLrHeader + len > rem || (t == 0 && len == 0) || (k == f0 && o != start) ||
            (k + 1 < f1 && k + 1 < p.n_headers && p.headers[k + 1] != o + kLrHeader + len);
    }
    if (bad) lr_raise(p.status, kLrBadInput);
  }
  for (uint64_t r = first; r < p.n_blocks; r += stride) {
    const uint64_t f0 = p.block_first[r], f1 = p.block_first[r + 1];
    const uint64_t start = (p.first_block + r) * kLrBlock, size = block_bytes(p.log_bytes, start);
    bool bad = f0 > f1 || f1 > p.n_headers;
    uint64_t pos = 0;
    if (!bad && f1 > f0) {
      const uint64_t o = p.headers[f1 - 1];
      bad = size < kLrHeader || o < start || o - start > size - kLrHeader;
      if (!bad) {
        uint32_t len, t;
        header_of(p, o, len, t);
        pos = o - start + kLrHeader + len;
        bad = pos > size;
      }
    }
    if (!bad) {
      const uint64_t rem = size - pos;
      uint32_t len = 0, t = 0;
      if (rem >= kLrHeader) header_of(p, start + pos, len, t);
      bool more;
      const uint64_t how = end_of_walk(rem, size, len, t, more);
      bad = more || p.block_end[2 * r] != how || p.block_end[2 * r + 1] != rem;
    }
    if (bad) lr_raise(p.status, kLrBadInput);
    p.cut[r] = bad ? 0 : f1;
  }
  if (first == 0) {
    if (p.block_first[0] != 0 || p.block_first[p.n_blocks] != p.n_headers) lr_raise(p.status, kLrBadInput);
    p.hdr[kHdrStop] = ~0ull;
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_plan_cut_kernel(LrPlan p) {
  if (*p.status != kLrOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kLrThreads;
  for (uint64_t k = global_index<kLrThreads>(); k < p.n_headers; k += stride)
    if (!p.ok[k]) atomicMin(reinterpret_cast<unsigned long long*>(&p.cut[p.headers[k] / kLrBlock - p.first_block]),
                            (unsigned long long)k);
}

// lead: the trailer bytes between the record before and this header.  ReadRecord takes
// physical_record_offset before ReadPhysicalRecord skips them, so LastRecordOffset() is off - lead.
__device__ __forceinline__ uint32_t lk_pack(uint32_t len, uint32_t kind, uint32_t lead, uint32_t t) {
  return len | kind << 16 | lead << 20 | t << 24;
}
__device__ __forceinline__ uint32_t lk_len(uint32_t lk) { return lk & 0xFFFFu; }
__device__ __forceinline__ uint32_t lk_kind(uint32_t lk) { return (lk >> 16) & 0xFu; }
__device__ __forceinline__ uint32_t lk_lead(uint32_t lk) { return (lk >> 20) & 0xFu; }
// sets in_fragmented_record whatever it was (a MIDDLE never does; a LAST leaves it false either way)
__device__ __forceinline__ bool is_setter(uint32_t kind) { return kind != kSlotNop && kind != kSlotMiddle && kind != kSlotTruncated; }

// the last value of a workgroup's lanes before this one that is not 0 (values
// grow with the lane where they are not 0), and the last of all; lds: kWaves words
template <uint32_t kWaves>
__device__ __forceinline__ void block_excl_last(uint64_t v, uint64_t* lds, uint64_t& excl, uint64_t& all) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t set = __ballot(v != 0), below = set & ((1ull << lane) - 1);
  // (every lane takes part in both shuffles: a lane that sat one out could not be read from)
  const uint64_t got = __shfl(v, below ? 63 - __builtin_clzll(below) : (int)lane);
  const uint64_t top = __shfl(v, set ? 63 - __builtin_clzll(set) : (int)lane);
  const uint64_t mine = below ? got : 0;
  if (lane == 0) lds[w] = set ? top : 0;
  __syncthreads();
  uint64_t before = 0;
  all = 0;
  for (uint32_t i = 0; i < kWaves; i++) {
    const uint64_t t = lds[i];
    if (i < w && t) before = t;
    if (t) all = t;
  }
  __syncthreads();
  excl = mine ? mine : before;
}

__global__ __launch_bounds__(kLrThreads) void lr_plan_classify_kernel(LrPlan p) {
  __shared__ uint64_t row[kLrWaves];
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  uint32_t kind = kSlotNop, len = 0, t = 0, lead = 0;
  uint64_t o = 0, end = 0;
  if (i < p.n_slots) {
    // the block of the slot: the last r in [0, n_blocks] with block_first[r] + r <= i
    uint64_t r = 0, hi = p.n_blocks + 1;
    while (hi - r > 1) {
      const uint64_t mid = r + ((hi - r) >> 1);
      if (p.block_first[mid] + mid <= i) r = mid; else hi = mid;
    }
    if (r == p.n_blocks) {  // the end of the file
      kind = kSlotEof;
      o = end = p.log_bytes;
    } else {
      const uint64_t k = i - r, f1 = p.block_first[r + 1], cut = p.cut[r];
      const uint64_t start = (p.first_block + r) * kLrBlock, bend = start + block_bytes(p.log_bytes, start);
      if (k < f1) {
        if (k <= cut) {
          o = p.headers[k];
          header_of(p, o, len, t);
          end = o + kLrHeader + len;
          if (r && k == p.block_first[r] && p.cut[r - 1] == k && p.block_end[2 * r - 2] == kEndTrailer)
            lead = (uint32_t)p.block_end[2 * r - 1];
          if (k == cut) {
            kind = kSlotChecksum;
            end = bend;
          } else if (o < p.initial_offset) {
            kind = kSlotBad;
          } else {
            kind = t >= 1 && t <= 6 ? t : kSlotUnknown;
          }
        }
      } else if (cut == f1) {
        const uint64_t how = p.block_end[2 * r];
        o = bend - p.block_end[2 * r + 1];
        end = bend;
        kind = how == kEndBadLength ? kSlotBadLength : how == kEndZeroHeader ? kSlotBad
               : how == kEndTruncated ? kSlotTruncated : kSlotNop;
      }
    }
    p.off[i] = o;
    p.end[i] = end;
    p.lk[i] = lk_pack(len, kind, lead, t);
    p.done[i] = 0;
    if (kind == kSlotEof) atomicMin(reinterpret_cast<unsigned long long*>(&p.hdr[kHdrStop]), (unsigned long long)i);
  }
  uint64_t excl, last, total;
  block_excl_last<kLrWaves>(is_setter(kind) ? i + 1 : 0, row, excl, last);
  block_excl_sum<kLrWaves>(kind == kSlotMiddle ? len : 0, row, excl, total);
  if (threadIdx.x == 0) {
    p.tiles[blockIdx.x] = last;
    p.tiles[(p.n_tiles + 1) + blockIdx.x] = total;
  }
}

// rows 0 and 1 of tiles: the last setter before each tile, the MIDDLE lengths before it
__global__ __launch_bounds__(kLrThreads) void lr_plan_scan_a_kernel(LrPlan p) {
  __shared__ uint64_t row[kLrWaves];
  if (*p.status != kLrOk) return;
  uint64_t last = 0, sum = 0;
  uint64_t* t0 = p.tiles;
  uint64_t* t1 = p.tiles + (p.n_tiles + 1);
  for (uint64_t c = 0; c < p.n_tiles; c += kLrThreads) {
    const uint64_t t = c + threadIdx.x;
    const uint64_t v0 = t < p.n_tiles ? t0[t] : 0, v1 = t < p.n_tiles ? t1[t] : 0;
    uint64_t e0, a0, e1, a1;
    block_excl_last<kLrWaves>(v0, row, e0, a0);
    block_excl_sum<kLrWaves>(v1, row, e1, a1);
    if (t < p.n_tiles) {
      t0[t] = e0 ? e0 : last;
      t1[t] = sum + e1;
    }
    if (a0) last = a0;
    sum += a1;
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_plan_state_kernel(LrPlan p) {
  __shared__ uint64_t row[kLrWaves];
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  const uint32_t lk = i < p.n_slots ? p.lk[i] : 0;
  uint64_t excl, last, mex, total;
  block_excl_last<kLrWaves>(is_setter(lk_kind(lk)) ? i + 1 : 0, row, excl, last);
  block_excl_sum<kLrWaves>(lk_kind(lk) == kSlotMiddle ? lk_len(lk) : 0, row, mex, total);
  if (i < p.n_slots) {
    p.setter[i] = excl ? excl : p.tiles[blockIdx.x];
    p.mex[i] = p.tiles[(p.n_tiles + 1) + blockIdx.x] + mex;
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_plan_scratch_kernel(LrPlan p) {
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  if (i >= p.n_slots) return;
  const uint64_t s = p.setter[i];
  uint64_t scr1 = 0;
  if (s) {
    const uint32_t lk = p.lk[s - 1];
    if (lk_kind(lk) == kSlotFirst) scr1 = 1 + lk_len(lk) + (p.mex[i] - p.mex[s - 1]);
  }
  p.scr1[i] = scr1;
  if (scr1 && lk_kind(p.lk[i]) == kSlotLast && i <= p.hdr[kHdrStop]) p.done[s - 1] = i + 1;
}

// What a slot yields, given ReadRecord's state on arrival.
struct Yield {
  uint32_t nrec, nrep, frag;
  uint64_t side;              // the assembled record's length (a completing LAST)
  uint64_t pbytes, lbytes, arg;  // ReadPhysicalRecord's report, then ReadRecord's; arg: the widened type of reason 10
  uint32_t preason, lreason;     // (0: none)
  uint64_t inner;             // a surviving fragment's offset in its record
  uint64_t last;              // 1 + the LAST slot of a surviving fragment's record
};

__device__ __forceinline__ void report(Yield& y, bool pass, uint32_t reason, uint64_t bytes) {
  if (!pass) return;
  y.lreason = reason;
  y.lbytes = bytes;
  y.nrep++;
}

__device__ __forceinline__ Yield yield_of(const LrPlan& p, uint64_t i) {
  Yield y = {};
  if (i > p.hdr[kHdrStop]) return y;
  const uint32_t lk = p.lk[i], kind = lk_kind(lk);
  const uint64_t len = lk_len(lk), o = p.off[i], end = p.end[i], scr1 = p.scr1[i], scr = scr1 - 1, init = p.initial_offset;
  const bool in = scr1 != 0;
  // ReportDrop's filter: end_of_buffer_offset_ - buffer_.size() - bytes >= initial_offset_, unsigned
  if (kind >= kSlotBadLength && o >= init) {
    y.preason = kind == kSlotBadLength ? 1 : kind == kSlotChecksum ? 2 : 3;
    y.pbytes = end - o;
    y.nrep = 1;
  }
  switch (kind) {
    case kSlotFull:
      report(y, in && scr && end - scr >= init, 4, scr);
      y.nrec = 1;
      break;
    case kSlotFirst:
      report(y, in && scr && end - scr >= init, 5, scr);
      y.frag = p.done[i] != 0;
      y.last = p.done[i];
      break;
    case kSlotMiddle:
      report(y, !in && end - len >= init, 7, len);
      if (in) {
        y.last = p.done[p.setter[i] - 1];
        y.frag = y.last != 0;
        y.inner = scr;
      }
      break;
    case kSlotLast:
      report(y, !in && end - len >= init, 8, len);
      if (in) {
        y.nrec = y.frag = 1;
        y.side = scr + len;
        y.inner = scr;
        y.last = i + 1;
      }
      break;
    case kSlotEof:
      report(y, in && end - scr >= init, 6, scr);
      break;
    case kSlotBad: case kSlotBadLength: case kSlotChecksum:
      report(y, in && end - scr >= init, 9, scr);
      break;
    case kSlotUnknown: {
      const uint64_t bytes = len + (in ? scr : 0);
      report(y, end - bytes >= init, 10, bytes);
      y.arg = (uint64_t)(uint32_t)(int32_t)(int8_t)(lk >> 24);  // char widened to unsigned int
      break;
    }
    default: break;
  }
  return y;
}

// rows 2..5 of tiles: records, reports, fragments, side bytes
__device__ __forceinline__ uint64_t* tile_row(const LrPlan& p, uint32_t row) { return p.tiles + row * (p.n_tiles + 1); }

__global__ __launch_bounds__(kLrThreads) void lr_plan_count_kernel(LrPlan p) {
  __shared__ uint64_t row[kLrWaves];
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  Yield y = {};
  if (i < p.n_slots) y = yield_of(p, i);
  // a tile's counts fit 16 bits each: one sum for the three
  uint64_t excl, counts, side;
  block_excl_sum<kLrWaves>(y.nrec | (uint64_t)y.nrep << 16 | (uint64_t)y.frag << 32, row, excl, counts);
  block_excl_sum<kLrWaves>(y.side, row, excl, side);
  if (threadIdx.x == 0) {
    tile_row(p, 2)[blockIdx.x] = counts & 0xFFFFu;
    tile_row(p, 3)[blockIdx.x] = (counts >> 16) & 0xFFFFu;
    tile_row(p, 4)[blockIdx.x] = counts >> 32;
    tile_row(p, 5)[blockIdx.x] = side;
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_plan_scan_b_kernel(LrPlan p) {
  __shared__ uint64_t row[kLrWaves];
  if (*p.status != kLrOk) return;
  uint64_t carry[4] = {0, 0, 0, 0};
  for (uint64_t c = 0; c < p.n_tiles; c += kLrThreads) {
    const uint64_t t = c + threadIdx.x;
    for (uint32_t q = 0; q < 4; q++) {
      uint64_t* tr = tile_row(p, 2 + q);
      uint64_t excl, total;
      block_excl_sum<kLrWaves>(t < p.n_tiles ? tr[t] : 0, row, excl, total);
      if (t < p.n_tiles) tr[t] = carry[q] + excl;
      carry[q] += total;
    }
  }
  if (threadIdx.x == 0) {
    const uint64_t stop = p.hdr[kHdrStop];
    p.hdr[kHdrRecords] = p.totals[0] = carry[0];
    p.hdr[kHdrEvents] = p.totals[1] = carry[1];
    p.hdr[kHdrFrags] = carry[2];
    p.hdr[kHdrSide] = p.totals[2] = carry[3];
    p.totals[3] = p.off[stop];
    p.hdr[kHdrSlots] = p.n_slots;
    p.hdr[kHdrLogBytes] = p.log_bytes;
    p.hdr[kHdrInitial] = p.initial_offset;
  }
}

// ---------------------------------------------------------------- emit

__global__ void lr_emit_check_kernel(LrEmitArgs a) {
  const uint64_t* h = a.p.hdr;
  if (h[kHdrSlots] != a.p.n_slots || h[kHdrLogBytes] != a.p.log_bytes || h[kHdrInitial] != a.p.initial_offset ||
      h[kHdrStop] >= a.p.n_slots ||
      h[kHdrFrags] > a.p.n_headers)
    lr_raise(a.p.status, kLrBadInput);  // not the scratch lsbm_log_read_plan_dev left for this log
  else if (h[kHdrRecords] > a.records_cap || h[kHdrEvents] > a.events_cap || h[kHdrSide] > a.side_cap)
    lr_raise(a.p.status, kLrNoRoom);
}

__global__ __launch_bounds__(kLrThreads) void lr_emit_slots_kernel(LrEmitArgs a) {
  __shared__ uint64_t row[kLrWaves];
  const LrPlan& p = a.p;
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  Yield y = {};
  if (i < p.n_slots) y = yield_of(p, i);
  uint64_t cx, sx, total;
  block_excl_sum<kLrWaves>(y.nrec | (uint64_t)y.nrep << 16 | (uint64_t)y.frag << 32, row, cx, total);
  block_excl_sum<kLrWaves>(y.side, row, sx, total);
  if (i >= p.n_slots) return;
  // (the caps hold for the plan's totals; a scratch that is not the plan's must not write past them either)
  const uint64_t rec = tile_row(p, 2)[blockIdx.x] + (cx & 0xFFFFu), ev = tile_row(p, 3)[blockIdx.x] + ((cx >> 16) & 0xFFFFu);
  sx += tile_row(p, 5)[blockIdx.x];
  p.fragex[i] = tile_row(p, 4)[blockIdx.x] + (cx >> 32);
  p.sidex[i] = sx;
  if (ev + y.nrep > a.events_cap || rec + y.nrec > a.records_cap) return;
  if (y.preason) {
    uint64_t* e = a.events + 4 * ev;
    e[0] = rec;
    e[1] = y.pbytes;
    e[2] = y.preason;
    e[3] = 0;
  }
  if (y.lreason) {
    uint64_t* e = a.events + 4 * (ev + (y.preason ? 1 : 0));
    e[0] = rec;
    e[1] = y.lbytes;
    e[2] = y.lreason;
    e[3] = y.lreason == 10 ? y.arg : 0;
  }
  if (y.nrec) {
    const uint32_t lk = p.lk[i];
    if (lk_kind(lk) == kSlotFull) {
      a.records[2 * rec] = p.log_at + p.off[i] + kLrHeader;
      a.records[2 * rec + 1] = lk_len(lk);
      a.last_record_offset[rec] = p.off[i] - lk_lead(lk);
    } else {  // a completing LAST: prospective_record_offset is its FIRST's
      const uint64_t f = p.setter[i] - 1;
      a.records[2 * rec] = a.side_at + sx;
      a.records[2 * rec + 1] = y.side;
      a.last_record_offset[rec] = p.off[f] - lk_lead(p.lk[f]);
    }
  }
}

__global__ __launch_bounds__(kLrThreads) void lr_emit_frags_kernel(LrEmitArgs a) {
  const LrPlan& p = a.p;
  if (*p.status != kLrOk) return;
  const uint64_t i = global_index<kLrThreads>();
  if (i >= p.n_slots) return;
  const Yield y = yield_of(p, i);
  if (!y.frag || p.fragex[i] >= p.n_headers) return;
  uint64_t* f = p.ftab + 3 * p.fragex[i];
  f[0] = p.sidex[y.last - 1] + y.inner;
  f[1] = p.off[i] + kLrHeader;
  f[2] = lk_len(p.lk[i]);
}

// A lane owns one 16-byte aligned chunk of the side area, finds the fragment
// its first byte belongs to by binary search in the fragment table (in side
// order: records in order, fragments in order) and either copies 16 source
// bytes (two 8-byte loads at any alignment, one aligned 16-byte store) or
// assembles the chunk byte by byte across fragments.  Only the area's first
// and last chunk leave as single bytes.
__global__ __launch_bounds__(kLrThreads) void lr_emit_move_kernel(LrEmitArgs a) {
  const LrPlan& p = a.p;
  if (*p.status != kLrOk) return;
  const uint64_t total = p.hdr[kHdrSide], nf = p.hdr[kHdrFrags];
  const uint64_t dst = reinterpret_cast<uint64_t>(a.out_image) + a.side_at, base = dst & ~(uint64_t)(kLrChunk - 1);
  const uint64_t n_chunks = total ? (dst + total - base + kLrChunk - 1) / kLrChunk : 0;
  const uint64_t stride = (uint64_t)gridDim.x * kLrThreads;
  const uint8_t* log = p.image + p.log_at;
  for (uint64_t c = global_index<kLrThreads>(); c < n_chunks; c += stride) {
    const uint64_t ca = base + c * kLrChunk;
    const uint64_t p0 = ca > dst ? ca - dst : 0, p1 = ca + kLrChunk - dst < total ? ca + kLrChunk - dst : total;
    uint64_t f = 0, hi = nf;  // the last fragment that starts at or before p0 (an empty one ties with its successor)
    while (hi - f > 1) {
      const uint64_t mid = f + ((hi - f) >> 1);
      if (p.ftab[3 * mid] <= p0) f = mid; else hi = mid;
    }
    uint64_t at = p.ftab[3 * f], src = p.ftab[3 * f + 1], len = p.ftab[3 * f + 2];
    const uint32_t i0 = (uint32_t)(dst + p0 - ca);
    if (at > p0 || src > p.log_bytes || len > p.log_bytes - src) continue;  // (not a plan's table)
    if (p1 - p0 == kLrChunk && p0 + kLrChunk <= at + len) {
      const uint8_t* s = log + src + (p0 - at);
      const uint64_t lo = load8(gptr(s, 0)), up = load8(gptr(s, 8));
      const u32x4 v = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)up, (uint32_t)(up >> 32)};
      *reinterpret_cast<gu32x4>(ca) = v;
      continue;
    }
    uint64_t lo = 0, up = 0;
    for (uint64_t q = p0; q < p1; q++) {
      while (q >= at + len && f + 1 < nf) {  // (q < total: there is a next fragment)
        f++;
        at = p.ftab[3 * f];
        src = p.ftab[3 * f + 1];
        len = p.ftab[3 * f + 2];
      }
      const uint64_t r = q - at;
      const uint64_t byte = r < len && src <= p.log_bytes && len <= p.log_bytes - src ? log[src + r] : 0;
      const uint32_t j = i0 + (uint32_t)(q - p0);
      if (j < 8) lo |= byte << (8 * j); else up |= byte << (8 * (j - 8));
    }
    if (p1 - p0 == kLrChunk) {
      const u32x4 v = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)up, (uint32_t)(up >> 32)};
      *reinterpret_cast<gu32x4>(ca) = v;
    } else {
      for (uint32_t j = i0; j < i0 + (uint32_t)(p1 - p0); j++)
        *reinterpret_cast<gu8>(ca + j) = (uint8_t)((j < 8 ? lo : up) >> (8 * (j & 7)));
    }
  }
}

}  // namespace

hipError_t launch_log_walk(const LrWalkArgs& a, int block_grid, int lane_grid, hipStream_t stream) {
  const dim3 block(kLrThreads);
  if (a.n_blocks) hipLaunchKernelGGL(lr_walk_kernel<false>, dim3(block_grid), block, 0, stream, a);
  hipLaunchKernelGGL(lr_walk_scan_kernel, dim3(1), block, 0, stream, a);
  if (a.n_blocks && a.headers) hipLaunchKernelGGL(lr_walk_kernel<true>, dim3(block_grid), block, 0, stream, a);
  hipLaunchKernelGGL(lr_walk_publish_kernel, dim3(lane_grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_log_plan(const LrPlan& p, int check_grid, hipStream_t stream) {
  const dim3 block(kLrThreads), tiles((uint32_t)p.n_tiles);
  hipLaunchKernelGGL(lr_plan_check_kernel, dim3(check_grid), block, 0, stream, p);
  if (p.n_headers) hipLaunchKernelGGL(lr_plan_cut_kernel, dim3(check_grid), block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_classify_kernel, tiles, block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_scan_a_kernel, dim3(1), block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_state_kernel, tiles, block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_scratch_kernel, tiles, block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_count_kernel, tiles, block, 0, stream, p);
  hipLaunchKernelGGL(lr_plan_scan_b_kernel, dim3(1), block, 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_log_emit(const LrEmitArgs& a, int move_grid, hipStream_t stream) {
  const dim3 block(kLrThreads), tiles((uint32_t)a.p.n_tiles);
  hipLaunchKernelGGL(lr_emit_check_kernel, dim3(1), dim3(1), 0, stream, a);
  hipLaunchKernelGGL(lr_emit_slots_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(lr_emit_frags_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(lr_emit_move_kernel, dim3(move_grid), block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
