// manifest_kernels.hip -- gfx950 kernels of the batched VersionEdit
// (include/lsbm_manifest.h): VersionEdit::DecodeFrom over many records at
// once, the entries of one long record found in parallel, and
// VersionEdit::EncodeTo for many edits at once.
//
// decode plan  mf_dec_first     one workgroup: the records' bounds, their
//                               lengths summed.  A position is a byte of the
//                               records laid end to end in the order given
//              mf_dec_parse     one lane per position: one tag group parsed as
//                               if it began there; where the next one would
//                               begin, or a terminal (span + verdict)
//              mf_dec_round     pointer doubling: next <- next[next]; a
//                               reachable position marks the one 2^k groups on
//              mf_dec_verdict   one lane per record: the terminal its chain reaches
//              mf_dec_flag      one lane per position: a reachable group of an
//                               OK record is a new file, a deleted file or a
//                               field (the last position wins its slot); a
//                               count per tile
//              mf_dec_scan      one workgroup: the tiles' running counts
//              mf_dec_publish   one lane per record: verdict, fields, counts
// decode emit  mf_dec_check     the caps against the totals
//              mf_dec_items     one lane per position: its item written at
//                               its slot; the keys moved by the whole wave
// encode plan  mf_enc_size      one lane per item: checked and sized
//              mf_scan_*        running sums of the sizes
//              mf_enc_edit      one lane per edit: checked and sized
//              mf_enc_publish   records, the total
// encode emit  mf_enc_check, mf_enc_edits, mf_enc_dels, mf_enc_news
//
// Every call has one status word, zeroed by the engine and raised by the
// check kernels; a kernel that writes an output leaves at once when it is
// set.  No spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "device_common.h"  // gptr, load8, store8, global_index, block_excl_sum, varint32
#include "manifest_types.h"

namespace lsbm {
namespace {

__device__ __forceinline__ void mf_raise(uint32_t* status, uint32_t code) { atomicMax(status, code); }

// GetVarint64Ptr (util/coding.cc:146-161): at most 10 bytes, the tenth byte's bits above 2^64 are lost
__device__ __forceinline__ bool varint64(const uint8_t* d, uint64_t& p, uint64_t limit, uint64_t& v) {
  uint64_t r = 0;
  for (uint32_t shift = 0; shift <= 63 && p < limit; shift += 7) {
    const uint64_t byte = d[p++];
    if (byte & 128u) {
      r |= (byte & 127u) << shift;
    } else {
      v = r | (byte << shift);
      return true;
    }
  }
  return false;
}

// GetLengthPrefixedSlice (util/coding.cc:182-192)
__device__ __forceinline__ bool get_slice(const uint8_t* d, uint64_t& p, uint64_t limit, uint64_t& off, uint64_t& len) {
  uint32_t n;
  if (!varint32(d, p, limit, n) || limit - p < n) return false;
  off = p;
  len = n;
  p += n;
  return true;
}

struct Group {
  uint32_t tag, type, level;
  uint64_t a, b;            // the group's first and second 64-bit number
  uint64_t k0, l0, k1, l1;  // its first and second slice: {offset in the image, length}
  uint64_t next;            // where it ends
};

// One turn of DecodeFrom's loop (lsbm/version_edit.cc:153-237) over
// d[p, end), p < end: 0 and the group, or the verdict it ends the record with.
__device__ __forceinline__ uint32_t parse_group(const uint8_t* d, uint64_t p, uint64_t end, Group& g) {
  uint32_t code = kVerOk;
  g.type = g.level = 0;
  g.a = g.b = g.k0 = g.l0 = g.k1 = g.l1 = 0;
  if (!varint32(d, p, end, g.tag)) return kVerInvalidTag;
  switch (g.tag) {
    case kTagComparator:
      if (!get_slice(d, p, end, g.k0, g.l0)) code = kVerComparator;
      break;
    case kTagLogNumber:
      if (!varint64(d, p, end, g.a)) code = kVerLogNumber;
      break;
    case kTagPrevLogNumber:
      if (!varint64(d, p, end, g.a)) code = kVerPrevLogNumber;
      break;
    case kTagNextFile:
      if (!varint64(d, p, end, g.a)) code = kVerNextFile;
      break;
    case kTagLastSequence:
      if (!varint64(d, p, end, g.a)) code = kVerLastSequence;
      break;
    case kTagDeletedFile:
      if (!(varint32(d, p, end, g.type) && varint32(d, p, end, g.level) && g.level < kMfLevels &&
            varint64(d, p, end, g.a)))
        code = kVerDeletedFile;
      else if (g.type >= kMfTypes)
        code = kVerTypeRange;
      break;
    case kTagNewFile:
      if (!(varint32(d, p, end, g.type) && varint32(d, p, end, g.level) && g.level < kMfLevels &&
            varint64(d, p, end, g.a) && varint64(d, p, end, g.b) && get_slice(d, p, end, g.k0, g.l0) &&
            get_slice(d, p, end, g.k1, g.l1)))
        code = kVerNewFile;
      else if (g.type >= kMfTypes)
        code = kVerTypeRange;
      break;
    case kTagWriteCursor:
      if (!varint64(d, p, end, g.a)) code = kVerWriteCursor;
      break;
    case kTagReadCursor:
      if (!varint64(d, p, end, g.a))
        code = kVerReadCursor;
      else if (g.a >= kMfLevels)
        code = kVerCursorRange;
      else if (!varint64(d, p, end, g.b))
        code = kVerReadCursor;
      break;
    default:
      code = kVerUnknownTag;
      break;
  }
  g.next = p;
  return code;
}

// the slot of a field group (its bit in the has mask, 6 + i for read cursor i)
__device__ __forceinline__ uint32_t slot_of(const Group& g) {
  switch (g.tag) {
    case kTagComparator: return 0;
    case kTagLogNumber: return 1;
    case kTagPrevLogNumber: return 2;
    case kTagNextFile: return 3;
    case kTagLastSequence: return 4;
    case kTagWriteCursor: return 5;
    default: return 6 + (uint32_t)g.a;
  }
}

// len bytes from s to d by the lanes of the wave together, for every lane that
// is active: 8 bytes a lane at any alignment, the last len % 8 as single
// bytes.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_copy(uint8_t* d, const uint8_t* s, uint64_t len, bool active) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t m = __ballot(active && len != 0); m; m &= m - 1) {
    const int l = __builtin_ctzll(m);
    const uint64_t dd = __shfl(reinterpret_cast<uint64_t>(d), l), ss = __shfl(reinterpret_cast<uint64_t>(s), l);
    const uint64_t n = __shfl(len, l), whole = n >> 3;
    for (uint64_t c = lane; c < whole; c += 64) store8(reinterpret_cast<gu8>(dd + 8 * c), load8(reinterpret_cast<gcu8>(ss + 8 * c)));
    const uint64_t i = 8 * whole + lane;
    if (i < n) *reinterpret_cast<gu8>(dd + i) = *reinterpret_cast<gcu8>(ss + i);
  }
}

// ---------------------------------------------------------------- decode

// the record of position g: the last r with rec_first[r] <= g (records of no bytes own no position)
__device__ __forceinline__ uint64_t rec_of(const MfDecode& a, uint64_t g) {
  uint64_t r = 0, hi = a.n;
  while (hi - r > 1) {
    const uint64_t mid = r + ((hi - r) >> 1);
    if (a.rec_first[mid] <= g) r = mid; else hi = mid;
  }
  return r;
}

__global__ __launch_bounds__(kMfThreads) void mf_dec_first_kernel(MfDecode a) {
  __shared__ uint64_t row[kMfWaves];
  uint64_t carry = 0;
  bool bad = false, big = false;
  for (uint64_t c = 0; c < a.n; c += kMfThreads) {
    const uint64_t r = c + threadIdx.x;
    uint64_t len = 0;
    if (r < a.n) {
      const uint64_t off = a.records[2 * r];
      len = a.records[2 * r + 1];
      if (off > a.image_size || len > a.image_size - off) bad = true, len = 0;
      if (len > a.longest_cap) big = true, len = 0;
    }
    uint64_t excl, total;
    block_excl_sum<kMfWaves>(len, row, excl, total);
    if (r < a.n) a.rec_first[r] = carry + excl;
    carry += total;  // (each record is at most longest_cap < 2^32 and n < 2^31: no wrap)
  }
  if (bad) mf_raise(a.status, kMfBadInput);
  if (big) mf_raise(a.status, kMfNoRoom);
  if (threadIdx.x == 0) {
    a.rec_first[a.n] = carry;
    if (carry > a.span_cap) mf_raise(a.status, kMfNoRoom);
    a.hdr[kMhN] = ~0ull;  // (no plan yet: mf_dec_publish signs it)
    a.hdr[kMhSpan] = carry;
    a.hdr[kMhNew] = a.hdr[kMhDel] = a.hdr[kMhKeyBytes] = 0;
  }
}

// A parse never reads past its own record's end: `end` is the record's, not the image's.
__global__ __launch_bounds__(kMfThreads) void mf_dec_parse_kernel(MfDecode a) {
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t g = global_index<kMfThreads>(); g < a.n * kMfSlots; g += stride) a.win[g] = 0;
  for (uint64_t g = global_index<kMfThreads>(); g < span; g += stride) {
    const uint64_t r = rec_of(a, g), first = a.rec_first[r], off = a.records[2 * r], end = off + a.records[2 * r + 1];
    Group grp;
    const uint32_t code = parse_group(a.image, off + (g - first), end, grp);
    a.nxt_a[g] = (uint32_t)(code ? span + code : grp.next == end ? span : first + (grp.next - off));
    a.kind[g] = (uint8_t)((code ? 0 : grp.tag) | (g == first ? 0x80u : 0u));
  }
}

// After round k the positions marked are the first 2^(k + 1) groups of every
// chain, and dst jumps 2^(k + 1) groups.  (A position marked in this very
// round may mark another: it lies on the chain too.)
__global__ __launch_bounds__(kMfThreads) void mf_dec_round_kernel(MfDecode a, const uint32_t* src, uint32_t* dst) {
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t g = global_index<kMfThreads>(); g < span; g += stride) {
    const uint32_t v = src[g];
    if (v >= span) {
      dst[g] = v;
      continue;
    }
    if (a.kind[g] & 0x80u) {
      const uint8_t k = a.kind[v];
      if (!(k & 0x80u)) a.kind[v] = k | 0x80u;
    }
    dst[g] = src[v];
  }
}

__global__ __launch_bounds__(kMfThreads) void mf_dec_verdict_kernel(MfDecode a, const uint32_t* fin) {
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t r = global_index<kMfThreads>(); r < a.n; r += stride) {
    uint32_t v = kVerOk;
    if (a.records[2 * r + 1]) {
      const uint64_t t = fin[a.rec_first[r]];
      v = t >= span ? (uint32_t)(t - span) : kVerInvalidTag;  // (the rounds reach every chain's end)
    }
    a.ver[r] = v;
  }
}

__device__ __forceinline__ uint64_t* mf_row(const MfDecode& a, uint32_t row) { return a.tiles + row * (a.n_tiles + 1); }

// one workgroup per tile of kMfThreads positions
__global__ __launch_bounds__(kMfThreads) void mf_dec_flag_kernel(MfDecode a) {
  __shared__ uint64_t row[kMfWaves];
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], g = global_index<kMfThreads>();
  uint64_t is_new = 0, is_del = 0, key_bytes = 0;
  if (g < span) {
    const uint32_t k = a.kind[g];
    uint32_t live = 0;
    if (k & 0x80u) {
      const uint64_t r = rec_of(a, g);
      if (a.ver[r] == kVerOk) {
        const uint64_t off = a.records[2 * r];
        Group grp;
        parse_group(a.image, off + (g - a.rec_first[r]), off + a.records[2 * r + 1], grp);
        if (grp.tag == kTagNewFile) {
          is_new = 1, live = kTagNewFile, key_bytes = grp.l0 + grp.l1;
        } else if (grp.tag == kTagDeletedFile) {
          is_del = 1, live = kTagDeletedFile;
        } else {
          atomicMax(reinterpret_cast<unsigned long long*>(&a.win[r * kMfSlots + slot_of(grp)]), (unsigned long long)(g + 1));
        }
      }
    }
    a.kind[g] = (uint8_t)live;
  }
  uint64_t excl, counts, bytes;
  block_excl_sum<kMfWaves>(is_new | is_del << 32, row, excl, counts);
  block_excl_sum<kMfWaves>(key_bytes, row, excl, bytes);
  if (threadIdx.x == 0) {
    mf_row(a, 0)[blockIdx.x] = counts & 0xFFFFFFFFu;
    mf_row(a, 1)[blockIdx.x] = counts >> 32;
    mf_row(a, 2)[blockIdx.x] = bytes;
  }
}

__global__ __launch_bounds__(kMfThreads) void mf_dec_scan_kernel(MfDecode a) {
  __shared__ uint64_t row[kMfWaves];
  if (*a.status != kMfOk) return;
  const uint64_t nt = (a.hdr[kMhSpan] + kMfThreads - 1) / kMfThreads;
  uint64_t carry[3] = {0, 0, 0};
  for (uint64_t c = 0; c < nt; c += kMfThreads) {
    const uint64_t t = c + threadIdx.x;
    for (uint32_t q = 0; q < 3; q++) {
      uint64_t* tr = mf_row(a, q);
      uint64_t excl, total;
      block_excl_sum<kMfWaves>(t < nt ? tr[t] : 0, row, excl, total);
      if (t < nt) tr[t] = carry[q] + excl;
      carry[q] += total;
    }
  }
  if (threadIdx.x == 0) {
    a.hdr[kMhNew] = carry[0];
    a.hdr[kMhDel] = carry[1];
    a.hdr[kMhKeyBytes] = carry[2];
  }
}

__global__ __launch_bounds__(kMfThreads) void mf_dec_publish_kernel(MfDecode a) {
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t r = global_index<kMfThreads>(); r < a.n; r += stride) {
    a.verdict[r] = a.ver[r];
    uint64_t* f = a.fields + r * kMfFieldWords;
    for (uint32_t w = 0; w < kMfFieldWords; w++) f[w] = 0;
    const uint64_t first = a.rec_first[r], off = a.records[2 * r], end = off + a.records[2 * r + 1];
    uint64_t has = 0, read_has = 0;
    for (uint32_t s = 0; s < kMfSlots; s++) {
      const uint64_t w = a.win[r * kMfSlots + s];
      if (!w) continue;
      Group grp;
      parse_group(a.image, off + (w - 1 - first), end, grp);
      if (s == 0) {
        f[kFCmpOff] = grp.k0;
        f[kFCmpLen] = grp.l0;
      } else if (s < 6) {
        f[kFLog + (s - 1)] = grp.a;
      } else {
        f[kFRead0 + (s - 6)] = grp.b;
      }
      if (s < 6) has |= 1ull << s; else read_has |= 1ull << (s - 6);
    }
    f[kFHas] = has;
    f[kFReadHas] = read_has;
    // the live items before the record's first position: the tile's count and the tile's positions before it
    uint64_t n_new = a.hdr[kMhNew], n_del = a.hdr[kMhDel];
    if (first < span) {
      const uint64_t t = first / kMfThreads;
      n_new = mf_row(a, 0)[t];
      n_del = mf_row(a, 1)[t];
      for (uint64_t g = t * kMfThreads; g < first; g++) {
        const uint32_t k = a.kind[g];
        n_new += k == kTagNewFile;
        n_del += k == kTagDeletedFile;
      }
    }
    a.new_first[r] = n_new;
    a.del_first[r] = n_del;
  }
  if (global_index<kMfThreads>() == 0) {
    a.new_first[a.n] = a.totals[0] = a.hdr[kMhNew];
    a.del_first[a.n] = a.totals[1] = a.hdr[kMhDel];
    a.totals[2] = a.hdr[kMhKeyBytes];
    a.hdr[kMhN] = a.n;
  }
}

__global__ void mf_dec_check_kernel(MfDecode a) {
  const uint64_t* h = a.hdr;
  if (h[kMhN] != a.n || h[kMhSpan] > a.span_cap || h[kMhNew] > h[kMhSpan] || h[kMhDel] > h[kMhSpan] ||
      h[kMhKeyBytes] > h[kMhSpan])
    mf_raise(a.status, kMfBadInput);  // not the scratch lsbm_edit_decode_plan_dev left for these records
  else if (h[kMhNew] > a.new_cap || h[kMhDel] > a.del_cap || h[kMhKeyBytes] > a.keys_cap)
    mf_raise(a.status, kMfNoRoom);
}

__global__ __launch_bounds__(kMfThreads) void mf_dec_items_kernel(MfDecode a) {
  __shared__ uint64_t row[kMfWaves];
  if (*a.status != kMfOk) return;
  const uint64_t span = a.hdr[kMhSpan], g = global_index<kMfThreads>();
  const uint32_t k = g < span ? a.kind[g] : 0;
  const bool is_new = k == kTagNewFile, is_del = k == kTagDeletedFile;
  Group grp = {};
  uint64_t r = 0;
  if (is_new || is_del) {
    r = rec_of(a, g);
    const uint64_t off = a.records[2 * r];
    parse_group(a.image, off + (g - a.rec_first[r]), off + a.records[2 * r + 1], grp);
  }
  uint64_t cx, kx, total;
  block_excl_sum<kMfWaves>((uint64_t)is_new | (uint64_t)is_del << 32, row, cx, total);
  block_excl_sum<kMfWaves>(is_new ? grp.l0 + grp.l1 : 0, row, kx, total);
  const uint64_t j = mf_row(a, 0)[blockIdx.x] + (cx & 0xFFFFFFFFu), d = mf_row(a, 1)[blockIdx.x] + (cx >> 32);
  kx += mf_row(a, 2)[blockIdx.x];
  // (the caps hold for the plan's totals; a scratch that is not the plan's must not write past them either)
  const bool put = is_new && j < a.new_cap && kx <= a.keys_cap && grp.l0 + grp.l1 <= a.keys_cap - kx;
  if (put) {
    uint64_t* o = a.new_items + kNewWords * j;
    o[0] = r, o[1] = grp.type, o[2] = grp.level, o[3] = grp.a, o[4] = grp.b;
    a.key_offsets[2 * j] = kx;
    a.key_offsets[2 * j + 1] = kx + grp.l0;
    if (j + 1 == a.hdr[kMhNew]) a.key_offsets[2 * j + 2] = kx + grp.l0 + grp.l1;
  }
  if (is_del && d < a.del_cap) {
    uint64_t* o = a.del_items + kDelWords * d;
    o[0] = r, o[1] = grp.type, o[2] = grp.level, o[3] = grp.a;
  }
  wave_copy(a.keys + kx, a.image + grp.k0, grp.l0, put);
  wave_copy(a.keys + kx + grp.l0, a.image + grp.k1, grp.l1, put);
}

__global__ void mf_dec_tail_kernel(MfDecode a) {
  if (*a.status == kMfOk && a.hdr[kMhNew] == 0) a.key_offsets[0] = 0;
}

// ---------------------------------------------------------------- running sums (encode)

struct MfScan {
  uint64_t* v;  // cnt + 1: values in, their exclusive running sums and the total out
  uint64_t cnt, n_tiles;
  uint64_t* tiles;
  const uint32_t* status;
};

__global__ __launch_bounds__(kMfThreads) void mf_scan_sum_kernel(MfScan s) {
  __shared__ uint64_t row[kMfWaves];
  if (*s.status != kMfOk) return;
  const uint64_t i = global_index<kMfThreads>();
  uint64_t excl, total;
  block_excl_sum<kMfWaves>(i < s.cnt ? s.v[i] : 0, row, excl, total);
  if (threadIdx.x == 0) s.tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMfThreads) void mf_scan_tiles_kernel(MfScan s) {
  __shared__ uint64_t row[kMfWaves];
  if (*s.status != kMfOk) return;
  uint64_t carry = 0;
  for (uint64_t c = 0; c < s.n_tiles; c += kMfThreads) {
    const uint64_t t = c + threadIdx.x;
    uint64_t excl, total;
    block_excl_sum<kMfWaves>(t < s.n_tiles ? s.tiles[t] : 0, row, excl, total);
    if (t < s.n_tiles) s.tiles[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) s.v[s.cnt] = carry;
}

__global__ __launch_bounds__(kMfThreads) void mf_scan_apply_kernel(MfScan s) {
  __shared__ uint64_t row[kMfWaves];
  if (*s.status != kMfOk) return;
  const uint64_t i = global_index<kMfThreads>();
  uint64_t excl, total;
  block_excl_sum<kMfWaves>(i < s.cnt ? s.v[i] : 0, row, excl, total);
  if (i < s.cnt) s.v[i] = s.tiles[blockIdx.x] + excl;
}

void launch_scan(uint64_t* v, uint64_t cnt, uint64_t* tiles, const uint32_t* status, hipStream_t stream) {
  MfScan s = {v, cnt, (cnt + kMfThreads - 1) / kMfThreads, tiles, status};
  const dim3 block(kMfThreads), grid((uint32_t)s.n_tiles);
  if (s.n_tiles) hipLaunchKernelGGL(mf_scan_sum_kernel, grid, block, 0, stream, s);
  hipLaunchKernelGGL(mf_scan_tiles_kernel, dim3(1), block, 0, stream, s);
  if (s.n_tiles) hipLaunchKernelGGL(mf_scan_apply_kernel, grid, block, 0, stream, s);
}

// ---------------------------------------------------------------- encode

__device__ __forceinline__ uint32_t vlen(uint64_t v) { return 1 + (63 - __builtin_clzll(v | 1)) / 7; }

// bytes stored one by one, none at or past lim
struct Put {
  uint8_t* d;
  uint64_t pos, lim;
  __device__ __forceinline__ void byte(uint32_t b) {
    if (pos < lim) d[pos] = (uint8_t)b;
    pos++;
  }
  __device__ __forceinline__ void varint(uint64_t v) {  // PutVarint64; PutVarint32 of a 32-bit value is the same bytes
    while (v >= 128) {
      byte((uint32_t)(v & 127) | 128);
      v >>= 7;
    }
    byte((uint32_t)v);
  }
};

// the edit of item j: the last e with first[e] <= j (first[n] is the item count)
__device__ __forceinline__ uint64_t edit_of(const uint64_t* first, uint64_t n, uint64_t j) {
  uint64_t e = 0, hi = n;
  while (hi - e > 1) {
    const uint64_t mid = e + ((hi - e) >> 1);
    if (first[mid] <= j) e = mid; else hi = mid;
  }
  return e;
}

// the first item of [lo, hi) whose type is t or more (the items of an edit are in type order)
__device__ __forceinline__ uint64_t type_bound(const uint64_t* items, uint32_t words, uint64_t lo, uint64_t hi, uint64_t t) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (items[words * mid + 1] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool first_ok(const uint64_t* first, uint64_t n, uint64_t e, uint64_t count) {
  return first[e] <= first[e + 1] && first[e + 1] <= count && (e != 0 || first[0] == 0) && (e + 1 != n || first[n] == count);
}

__device__ __forceinline__ uint64_t head_bytes(const uint64_t* f) {
  const uint64_t has = f[kFHas];
  uint64_t b = 0;
  if (has & 1) b += 1 + vlen(f[kFCmpLen]) + f[kFCmpLen];
  for (uint32_t s = 1; s < 5; s++)
    if (has >> s & 1) b += 1 + vlen(f[kFLog + (s - 1)]);
  return b;
}
__device__ __forceinline__ uint64_t tail_bytes(const uint64_t* f) {
  uint64_t b = 1 + vlen(f[kFWriteCursor]);
  for (uint32_t i = 0; i < kMfLevels; i++) b += 2 + vlen(f[kFRead0 + i]);
  return b;
}

__global__ __launch_bounds__(kMfThreads) void mf_enc_size_kernel(MfEncode a) {
  const uint64_t first = global_index<kMfThreads>(), stride = (uint64_t)gridDim.x * kMfThreads;
  bool bad = false;
  for (uint64_t e = first; e < a.n; e += stride) {
    const uint64_t* f = a.fields + e * kMfFieldWords;
    if (!first_ok(a.del_first, a.n, e, a.n_del) || !first_ok(a.new_first, a.n, e, a.n_new)) bad = true;
    if ((f[kFHas] & 1) && (f[kFCmpLen] >> 32 || f[kFCmpOff] > a.names_size || f[kFCmpLen] > a.names_size - f[kFCmpOff]))
      bad = true;
  }
  if (a.n == 0 && first == 0 && (a.n_del || a.n_new)) bad = true;
  if (first == 0) a.hdr[kMhN] = ~0ull;  // (no plan yet: mf_enc_publish signs it)
  for (uint64_t j = first; j < a.n_del; j += stride) {
    const uint64_t* it = a.del_items + kDelWords * j;
    uint64_t size = 0;
    if (it[0] >= a.n || it[1] >= kMfTypes || it[2] >= kMfLevels) {
      bad = true;
    } else {
      size = 3 + vlen(it[3]);
      // std::set<pair<level, number>> per type: strictly ascending inside the edit (the neighbour's own lane checks its edit)
      if (j + 1 < a.n_del && it[4] == it[0] &&
          !(it[1] < it[5] || (it[1] == it[5] && (it[2] < it[6] || (it[2] == it[6] && it[3] < it[7])))))
        bad = true;
    }
    a.pd[j] = size;
  }
  for (uint64_t j = first; j < a.n_new; j += stride) {
    const uint64_t* it = a.new_items + kNewWords * j;
    const uint64_t k0 = a.key_offsets[2 * j], k1 = a.key_offsets[2 * j + 1], k2 = a.key_offsets[2 * j + 2];
    uint64_t size = 0;
    if (it[0] >= a.n || it[1] >= kMfTypes || it[2] >= kMfLevels || k0 > k1 || k1 > k2 || k2 > a.keys_size ||
        (k1 - k0) >> 32 || (k2 - k1) >> 32) {
      bad = true;
    } else {
      size = 3 + vlen(it[3]) + vlen(it[4]) + vlen(k1 - k0) + (k1 - k0) + vlen(k2 - k1) + (k2 - k1);
      if (j + 1 < a.n_new && it[5] == it[0] && it[1] > it[6]) bad = true;
    }
    a.pn[j] = size;
  }
  if (bad) mf_raise(a.status, kMfBadInput);
}

// (after the first arrays are known good) an item's record is the edit that lists it
__global__ __launch_bounds__(kMfThreads) void mf_enc_owner_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t first = global_index<kMfThreads>(), stride = (uint64_t)gridDim.x * kMfThreads;
  bool bad = false;
  for (uint64_t j = first; j < a.n_del; j += stride)
    if (a.del_items[kDelWords * j] != edit_of(a.del_first, a.n, j)) bad = true;
  for (uint64_t j = first; j < a.n_new; j += stride)
    if (a.new_items[kNewWords * j] != edit_of(a.new_first, a.n, j)) bad = true;
  if (bad) mf_raise(a.status, kMfBadInput);
}

__global__ __launch_bounds__(kMfThreads) void mf_enc_edit_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t e = global_index<kMfThreads>(); e < a.n; e += stride) {
    const uint64_t* f = a.fields + e * kMfFieldWords;
    a.pe[e] = head_bytes(f) + (a.pd[a.del_first[e + 1]] - a.pd[a.del_first[e]]) +
              (a.pn[a.new_first[e + 1]] - a.pn[a.new_first[e]]) + tail_bytes(f);
  }
}

__global__ __launch_bounds__(kMfThreads) void mf_enc_publish_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kMfThreads;
  for (uint64_t e = global_index<kMfThreads>(); e < a.n; e += stride) {
    a.records[2 * e] = a.out_at + a.pe[e];
    a.records[2 * e + 1] = a.pe[e + 1] - a.pe[e];
  }
  if (global_index<kMfThreads>() == 0) {
    a.totals[0] = a.pe[a.n];
    a.hdr[kMhN] = a.n;
    a.hdr[kMhNew] = a.n_new;
    a.hdr[kMhDel] = a.n_del;
    a.hdr[kMhBytes] = a.pe[a.n];
  }
}

__global__ void mf_enc_check_kernel(MfEncode a) {
  const uint64_t* h = a.hdr;
  if (h[kMhN] != a.n || h[kMhNew] != a.n_new || h[kMhDel] != a.n_del || h[kMhBytes] != a.pe[a.n])
    mf_raise(a.status, kMfBadInput);  // not the scratch lsbm_edit_encode_plan_dev left for these edits
  else if (h[kMhBytes] > a.out_cap)
    mf_raise(a.status, kMfNoRoom);
}

__global__ __launch_bounds__(kMfThreads) void mf_enc_edits_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kMfThreads, lim = a.out_at + a.hdr[kMhBytes];
  for (uint64_t e = global_index<kMfThreads>(); e < a.n; e += stride) {
    const uint64_t* f = a.fields + e * kMfFieldWords;
    const uint64_t has = f[kFHas];
    Put p = {a.image, a.out_at + a.pe[e], lim};
    if (has & 1) {  // (a name is a few bytes: one lane)
      p.byte(kTagComparator);
      p.varint(f[kFCmpLen]);
      for (uint64_t i = 0; i < f[kFCmpLen]; i++) p.byte(a.names[f[kFCmpOff] + i]);
    }
    const uint32_t tags[4] = {kTagLogNumber, kTagPrevLogNumber, kTagNextFile, kTagLastSequence};
#pragma unroll
    for (uint32_t s = 0; s < 4; s++)
      if (has >> (s + 1) & 1) {
        p.byte(tags[s]);
        p.varint(f[kFLog + s]);
      }
    p.pos = a.out_at + a.pe[e + 1] - tail_bytes(f);
    p.byte(kTagWriteCursor);
    p.varint(f[kFWriteCursor]);
    for (uint32_t i = 0; i < kMfLevels; i++) {
      p.byte(kTagReadCursor);
      p.byte(i);
      p.varint(f[kFRead0 + i]);
    }
  }
}

// Inside an edit: for t = 0..3 the deleted files of type t, then the new files of type t.
__global__ __launch_bounds__(kMfThreads) void mf_enc_dels_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kMfThreads, lim = a.out_at + a.hdr[kMhBytes];
  for (uint64_t j = global_index<kMfThreads>(); j < a.n_del; j += stride) {
    const uint64_t* it = a.del_items + kDelWords * j;
    const uint64_t e = edit_of(a.del_first, a.n, j), n0 = a.new_first[e];
    const uint64_t nb = type_bound(a.new_items, kNewWords, n0, a.new_first[e + 1], it[1]);
    Put p = {a.image, a.out_at + a.pe[e] + head_bytes(a.fields + e * kMfFieldWords) + (a.pd[j] - a.pd[a.del_first[e]]) +
                          (a.pn[nb] - a.pn[n0]), lim};
    p.byte(kTagDeletedFile);
    p.byte((uint32_t)it[1]);
    p.byte((uint32_t)it[2]);
    p.varint(it[3]);
  }
}

__global__ __launch_bounds__(kMfThreads) void mf_enc_news_kernel(MfEncode a) {
  if (*a.status != kMfOk) return;
  const uint64_t stride = (uint64_t)gridDim.x * kMfThreads, lim = a.out_at + a.hdr[kMhBytes];
  for (uint64_t base = (uint64_t)blockIdx.x * kMfThreads; base < a.n_new; base += stride) {  // (the whole wave turns together)
    const uint64_t j = base + threadIdx.x;
    const bool on = j < a.n_new;
    uint64_t k0 = 0, l0 = 0, l1 = 0, at0 = 0, at1 = 0;
    if (on) {
      const uint64_t* it = a.new_items + kNewWords * j;
      const uint64_t e = edit_of(a.new_first, a.n, j), d0 = a.del_first[e];
      const uint64_t db = type_bound(a.del_items, kDelWords, d0, a.del_first[e + 1], it[1] + 1);
      k0 = a.key_offsets[2 * j];
      l0 = a.key_offsets[2 * j + 1] - k0;
      l1 = a.key_offsets[2 * j + 2] - k0 - l0;
      Put p = {a.image, a.out_at + a.pe[e] + head_bytes(a.fields + e * kMfFieldWords) + (a.pd[db] - a.pd[d0]) +
                            (a.pn[j] - a.pn[a.new_first[e]]), lim};
      p.byte(kTagNewFile);
      p.byte((uint32_t)it[1]);
      p.byte((uint32_t)it[2]);
      p.varint(it[3]);
      p.varint(it[4]);
      p.varint(l0);
      at0 = p.pos;
      p.pos += l0;
      p.varint(l1);
      at1 = p.pos;
    }
    wave_copy(a.image + at0, a.keys + k0, l0, on && at0 <= lim && l0 <= lim - at0);
    wave_copy(a.image + at1, a.keys + k0 + l0, l1, on && at1 <= lim && l1 <= lim - at1);
  }
}

}  // namespace

hipError_t launch_edit_decode_plan(const MfDecode& a, int lane_grid, int rec_grid, hipStream_t stream) {
  const dim3 block(kMfThreads), tiles((uint32_t)a.n_tiles);
  hipLaunchKernelGGL(mf_dec_first_kernel, dim3(1), block, 0, stream, a);
  hipLaunchKernelGGL(mf_dec_parse_kernel, dim3(lane_grid), block, 0, stream, a);
  uint32_t* src = a.nxt_a;
  uint32_t* dst = a.nxt_b;
  for (uint32_t k = 0; k < a.rounds && a.n_tiles; k++) {
    hipLaunchKernelGGL(mf_dec_round_kernel, dim3(lane_grid), block, 0, stream, a, src, dst);
    std::swap(src, dst);
  }
  hipLaunchKernelGGL(mf_dec_verdict_kernel, dim3(rec_grid), block, 0, stream, a, src);
  if (a.n_tiles) hipLaunchKernelGGL(mf_dec_flag_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(mf_dec_scan_kernel, dim3(1), block, 0, stream, a);
  hipLaunchKernelGGL(mf_dec_publish_kernel, dim3(rec_grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_edit_decode_emit(const MfDecode& a, hipStream_t stream) {
  const dim3 block(kMfThreads), tiles((uint32_t)a.n_tiles);
  hipLaunchKernelGGL(mf_dec_check_kernel, dim3(1), dim3(1), 0, stream, a);
  if (a.n_tiles) hipLaunchKernelGGL(mf_dec_items_kernel, tiles, block, 0, stream, a);
  hipLaunchKernelGGL(mf_dec_tail_kernel, dim3(1), dim3(1), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_edit_encode_plan(const MfEncode& a, int grid, hipStream_t stream) {
  const dim3 block(kMfThreads);
  hipLaunchKernelGGL(mf_enc_size_kernel, dim3(grid), block, 0, stream, a);
  hipLaunchKernelGGL(mf_enc_owner_kernel, dim3(grid), block, 0, stream, a);
  launch_scan(a.pd, a.n_del, a.tiles, a.status, stream);
  launch_scan(a.pn, a.n_new, a.tiles, a.status, stream);
  hipLaunchKernelGGL(mf_enc_edit_kernel, dim3(grid), block, 0, stream, a);
  launch_scan(a.pe, a.n, a.tiles, a.status, stream);
  hipLaunchKernelGGL(mf_enc_publish_kernel, dim3(grid), block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_edit_encode_emit(const MfEncode& a, int grid, hipStream_t stream) {
  const dim3 block(kMfThreads);
  hipLaunchKernelGGL(mf_enc_check_kernel, dim3(1), dim3(1), 0, stream, a);
  hipLaunchKernelGGL(mf_enc_edits_kernel, dim3(grid), block, 0, stream, a);
  hipLaunchKernelGGL(mf_enc_dels_kernel, dim3(grid), block, 0, stream, a);
  hipLaunchKernelGGL(mf_enc_news_kernel, dim3(grid), block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
