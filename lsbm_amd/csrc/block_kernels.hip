// block_kernels.hip -- gfx950 kernels of the batched SSTable block reader
// (include/lsbm_block.h): Block::Iter of table/block.cc for many blocks.
//
// block_walk_kernel<false>  block_scan: per block the entry count, the bytes of
//                           the fully expanded keys, the value bytes and the
//                           reference's status.
// block_walk_kernel<true>   block_decode: the same walk, then the keys, key
//                           offsets and value slices written into the
//                           caller's windows.
// block_seek_kernel         Block::Iter::Seek for many (block, target) pairs,
//                           one query per lane.
//
// One wave per block.  A block of at most kBlockTileBytes is staged into the
// wave's LDS tile with 16-B loads and walked from there; a larger one (an
// index block) is walked from global memory by the same code, templated on
// the pointer type.  Fast path: one lane per restart interval, in chunks of
// 64 intervals; it holds only if restart[0] == 0, the restart offsets rise
// strictly below restarts_, every interval's walk lands exactly on the next
// restart point and every interval starts with shared == 0.  Otherwise lane 0
// walks the block from restart[0] as ParseNextKey does (table/block.cc:288-315).
//
// Every byte of a block is untrusted: all offsets are block-relative 32-bit
// values checked against restarts_ before a byte is read, every loop advances
// its offset by at least 3 bytes (an entry header) or halves a range, and no
// store leaves the caller's windows.  No spin-waits, no cross-workgroup state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_types.h"
#include "device_common.h"  // gcu8, gu8, lu8, u32x4, gptr, gwptr, wave_phase, wave_sum, wave_incl_scan, varint32

namespace lsbm {
namespace {

template <class P>
__device__ __forceinline__ uint32_t le32(P d, uint32_t o) {  // DecodeFixed32, any alignment
  return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24);
}

struct Hdr {
  uint32_t shared, ns, vl;
  uint32_t kp;  // offset of the key delta
};

// DecodeEntry (table/block.cc:111-132) at offset p, limit = restarts_.  The
// last check adds in 64 bits: where the reference's 32-bit sum wraps it reads
// out of bounds; here that entry fails.
template <class P>
__device__ __forceinline__ bool decode_entry(P d, uint32_t p, uint32_t limit, Hdr& h) {
  if (p > limit || limit - p < 3) return false;
  uint32_t a = d[p], b = d[p + 1], c = d[p + 2];
  if ((a | b | c) < 128u) {
    p += 3;
  } else {
    if (!varint32(d, p, limit, a)) return false;
    if (!varint32(d, p, limit, b)) return false;
    if (!varint32(d, p, limit, c)) return false;
  }
  if ((uint64_t)(limit - p) < (uint64_t)b + (uint64_t)c) return false;
  h.shared = a;
  h.ns = b;
  h.vl = c;
  h.kp = p;
  return true;
}

struct Tot {
  uint64_t n, kb, vb;
};

// A lane's copy of its walk's previous key, first kKeyCache bytes, in LDS: a
// key's shared prefix is then copied from there instead of being read back
// from the output behind the stores that wrote it.  Dword rows interleaved
// over the 64 lanes (byte i of lane l at row i / 4, column 4 l + i % 4).
constexpr uint32_t kKeyCache = 64;
constexpr uint32_t kKeyCacheWave = kKeyCache * 64;
__device__ __forceinline__ uint32_t kc_idx(uint32_t i) { return (i >> 2) * 256u + (i & 3u); }

// Where a walk's entries go.  Entry t.n of the walk is entry e0 + t.n of the
// output, its key starts at key byte k0 + t.kb.  The windows' ends are
// checked again at every entry (the totals were checked before the walk).
struct Writer {
  bool on;
  lu8 kc;  // this lane's key cache
  uint64_t e0, e_end, k0, k_end;
  uint64_t block_off;
  uint8_t* keys;
  uint64_t* key_offsets;
  uint64_t* values;
};

template <class P>
__device__ __forceinline__ void write_entry(const Writer& w, P d, const Tot& t, uint64_t klen_prev, const Hdr& h) {
  const uint64_t e = w.e0 + t.n, ko = w.k0 + t.kb, klen = (uint64_t)h.shared + h.ns;
  if (e >= w.e_end || ko > w.k_end || klen > w.k_end - ko) return;
  const gu8 out = reinterpret_cast<gu8>(reinterpret_cast<uint64_t>(w.keys));
  const uint64_t kprev = ko - klen_prev;  // this walk's previous key (shared <= klen_prev)
  // the shared prefix: its first kKeyCache bytes from the lane's copy of the
  // previous key in LDS, the rest (long keys) from the output just written
  const uint32_t cs = h.shared < kKeyCache ? h.shared : kKeyCache;
  for (uint32_t i = 0; i < cs; i++) out[ko + i] = w.kc[kc_idx(i)];
  for (uint32_t i = kKeyCache; i < h.shared; i++) out[ko + i] = out[kprev + i];
  for (uint32_t i = 0; i < h.ns; i++) {
    const uint8_t b = d[h.kp + i];
    out[ko + h.shared + i] = b;
    if ((uint64_t)h.shared + i < kKeyCache) w.kc[kc_idx(h.shared + i)] = b;
  }
  w.key_offsets[e + 1] = ko + klen;
  w.values[2 * e] = w.block_off + h.kp + h.ns;
  w.values[2 * e + 1] = h.vl;
}

// One restart interval [p, end): true if its first entry has shared == 0,
// every entry decodes with shared <= the previous key's length, and the walk
// lands exactly on end.
template <class P>
__device__ __forceinline__ bool walk_interval(P d, uint32_t p, uint32_t end, uint32_t limit, Tot& t, const Writer& w) {
  uint64_t klen = 0;
  while (p < end) {
    Hdr h;
    if (!decode_entry(d, p, limit, h)) return false;
    if (h.shared > klen) return false;  // (the first entry: shared != 0)
    if (w.on) write_entry(w, d, t, klen, h);
    klen = (uint64_t)h.shared + h.ns;
    t.n++;
    t.kb += klen;
    t.vb += h.vl;
    p = h.kp + h.ns + h.vl;  // <= limit (decode_entry)
  }
  return p == end;
}

// SeekToFirst, then Next until !Valid (table/block.cc:288-315), from offset p.
template <class P>
__device__ __forceinline__ uint32_t walk_sequential(P d, uint32_t p, uint32_t limit, Tot& t, const Writer& w) {
  uint64_t klen = 0;
  while (p < limit) {
    Hdr h;
    if (!decode_entry(d, p, limit, h) || klen < h.shared) return kBlkBadEntry;
    if (w.on) write_entry(w, d, t, klen, h);
    klen = (uint64_t)h.shared + h.ns;
    t.n++;
    t.kb += klen;
    t.vb += h.vl;
    p = h.kp + h.ns + h.vl;
  }
  return kBlkOk;
}

// The restart interval of lane `lane` in the chunk starting at interval c0:
// false if it breaks the fast path's ordering rules.
template <class P>
__device__ __forceinline__ bool interval_of(P d, uint32_t restarts, uint32_t nr, uint32_t i, uint32_t& s, uint32_t& e) {
  s = le32(d, restarts + 4u * i);
  e = i + 1 < nr ? le32(d, restarts + 4u * (i + 1)) : restarts;
  return (i != 0 || s == 0) && s < e && e <= restarts;
}

// One block [d, d + size) by one wave.  Returns the status; tot is valid in
// every lane.  kDecode: after the totals, the block's windows are checked and
// the entries written.
template <bool kDecode, class P>
__device__ __forceinline__ uint32_t walk_block(P d, uint32_t size, uint64_t block_off, uint64_t blk, const BlockWalkArgs& a,
                                               uint32_t lane, lu8 kc, Tot& tot) {
  tot = Tot{0, 0, 0};
  const uint32_t nr = le32(d, size - 4);
  if (nr > (size - 4) / 4) return kBlkBadContents;  // Block::Block, table/block.cc:33-36
  const uint32_t restarts = size - (1 + nr) * 4;
  Writer w = {};
  uint32_t status = kBlkOk;
  bool fast = nr != 0;
  // pass 1: validity and totals
  for (uint32_t c0 = 0; fast && c0 < nr; c0 += 64) {
    const uint32_t i = c0 + lane;
    Tot t = {0, 0, 0};
    bool good = true;
    if (i < nr) {
      uint32_t s, e;
      good = interval_of(d, restarts, nr, i, s, e);
      if (good) good = walk_interval(d, s, e, restarts, t, w);
    }
    if (__ballot(!good) != 0ull) {
      fast = false;
      break;
    }
    tot.n += wave_sum(t.n);
    tot.kb += wave_sum(t.kb);
    tot.vb += wave_sum(t.vb);
  }
  if (!fast && nr != 0) {
    Tot t = {0, 0, 0};
    uint32_t st = kBlkOk;
    if (lane == 0) st = walk_sequential(d, le32(d, restarts), restarts, t, w);
    status = (uint32_t)__builtin_amdgcn_readfirstlane((int)st);
    tot.n = wave_sum(t.n);
    tot.kb = wave_sum(t.kb);
    tot.vb = wave_sum(t.vb);
  }
  if (!kDecode) return status;
  // the block's windows
  const uint64_t e0 = a.entry_base[blk], e1 = a.entry_base[blk + 1];
  const uint64_t k0 = a.key_base[blk], k1 = a.key_base[blk + 1];
  if (e1 < e0 || k1 < k0 || e1 > a.entries_cap || k1 > a.keys_cap || tot.n > e1 - e0 || tot.kb > k1 - k0)
    return kBlkNoRoom;
  w.on = true;
  w.kc = kc;
  w.e_end = e1;
  w.k_end = k1;
  w.block_off = block_off;
  w.keys = a.keys;
  w.key_offsets = a.key_offsets;
  w.values = a.values;
  if (lane == 0) a.key_offsets[e0] = k0;
  if (nr == 0) return status;
  if (fast) {
    uint64_t ce = e0, ck = k0;  // running carry over the chunks
    for (uint32_t c0 = 0; c0 < nr; c0 += 64) {
      const uint32_t i = c0 + lane;
      Tot t = {0, 0, 0};
      uint32_t s = 0, e = 0;
      Writer off = {};
      if (i < nr) {
        interval_of(d, restarts, nr, i, s, e);
        walk_interval(d, s, e, restarts, t, off);
      }
      const uint64_t in = wave_incl_scan(t.n, lane), ik = wave_incl_scan(t.kb, lane);
      w.e0 = ce + in - t.n;
      w.k0 = ck + ik - t.kb;
      if (i < nr) {
        Tot t2 = {0, 0, 0};
        walk_interval(d, s, e, restarts, t2, w);
      }
      ce += __shfl(in, 63);
      ck += __shfl(ik, 63);
    }
  } else if (lane == 0) {
    Tot t = {0, 0, 0};
    w.e0 = e0;
    w.k0 = k0;
    walk_sequential(d, le32(d, restarts), restarts, t, w);
  }
  return status;
}

template <bool kDecode>
__global__ __launch_bounds__(kBlockThreads) void block_walk_kernel(BlockWalkArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tiles[kBlockWaves][kBlockTileAlloc];
  __shared__ __attribute__((aligned(16))) uint8_t kcache[kDecode ? kBlockWaves * kKeyCacheWave : 16];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* tile = tiles[wv];
  const lu8 kc = (lu8)(kcache + (kDecode ? wv * kKeyCacheWave + lane * 4u : 0u));
  const uint64_t nwaves = (uint64_t)gridDim.x * kBlockWaves;
  const uint64_t img = reinterpret_cast<uint64_t>(a.image);
  for (uint64_t blk = (uint64_t)blockIdx.x * kBlockWaves + wv; blk < a.n; blk += nwaves) {
    const uint64_t off = a.handles[2 * blk], size = a.handles[2 * blk + 1];
    Tot tot = {0, 0, 0};
    uint32_t status;
    // a handle not wholly inside the image, or of 4 GiB and more: bad block
    // contents (library-defined); size < 4: Block::Block, table/block.cc:30-31
    if (off > a.image_size || size > a.image_size - off || size > 0xffffffffull || size < 4) {
      status = kBlkBadContents;
    } else if (size <= kBlockTileBytes) {
      // stage [g, g + size) at its 16-B phase: aligned 16-B loads for chunks
      // inside the image, single bytes for a chunk that straddles its ends
      const uint64_t g = img + off, a0 = g & ~15ull;
      const uint32_t phase = (uint32_t)(g - a0);
      const uint32_t nch = (phase + (uint32_t)size + 15u) >> 4;
      for (uint32_t c = lane; c < nch; c += 64) {
        const uint64_t ca = a0 + 16ull * c;
        if (ca >= img && ca + 16 <= img + a.image_size) {
          *reinterpret_cast<u32x4*>(tile + 16u * c) = *reinterpret_cast<gcu32x4>(ca);
        } else {
          for (uint32_t j = 0; j < 16; j++)
            if (ca + j >= img && ca + j < img + a.image_size) tile[16u * c + j] = *reinterpret_cast<gcu8>(ca + j);
        }
      }
      wave_phase();
      status = walk_block<kDecode>(static_cast<const uint8_t*>(tile + phase), (uint32_t)size, off, blk, a, lane, kc, tot);
      wave_phase();  // (the next block's staging writes after these reads)
    } else {
      status = walk_block<kDecode>(reinterpret_cast<gcu8>(img + off), (uint32_t)size, off, blk, a, lane, kc, tot);
    }
    if (kDecode && status == kBlkBadContents && lane == 0) {
      // no entries: the block's (empty) run of key offsets still starts at its window
      const uint64_t e0 = a.entry_base[blk], e1 = a.entry_base[blk + 1];
      if (e0 <= e1 && e1 <= a.entries_cap) a.key_offsets[e0] = a.key_base[blk];
    }
    if (lane == 0) {
      a.status[blk] = status;
      if (a.counts) {
        a.counts[3 * blk] = tot.n;
        a.counts[3 * blk + 1] = tot.kb;
        a.counts[3 * blk + 2] = tot.vb;
      }
    }
  }
}

// ---- Seek ----

// What Seek needs of the current key against the target without holding the
// key: its length, the length of its common prefix with the target (at most
// min(klen, tlen)), the order of the first differing byte, and for the
// internal comparator the key's bytes at the positions of the target's tag
// [tlen - 8, tlen) (they are the key's tag when klen == tlen).  A key is its
// predecessor's first `shared` bytes plus a delta, so all four follow from the
// predecessor's.
struct KeyState {
  uint64_t klen, lcp;
  int sgn;
  uint64_t tail;
};

template <class P>
__device__ __forceinline__ void advance(KeyState& k, P d, const Hdr& h, gcu8 t, uint64_t tlen, bool internal) {
  const uint64_t klen = (uint64_t)h.shared + h.ns;
  if (h.shared <= k.lcp) {
    // the shared prefix matches the target; compare the delta from there on
    uint64_t l = h.shared;
    const uint64_t m = klen < tlen ? klen : tlen;
    int sgn = 0;
    while (l < m) {
      const uint32_t kb = d[h.kp + (uint32_t)(l - h.shared)], tb = t[l];
      if (kb != tb) {
        sgn = kb < tb ? -1 : 1;
        break;
      }
      l++;
    }
    k.lcp = l;
    k.sgn = sgn;
  }  // else: the first difference lies inside the shared prefix, as before
  if (internal && tlen >= 8) {
    const uint64_t p0 = tlen - 8;
    for (uint32_t i = 0; i < 8; i++) {
      const uint64_t pos = p0 + i;
      if (pos >= h.shared && pos < klen) {
        const uint64_t b = d[h.kp + (uint32_t)(pos - h.shared)];
        k.tail = (k.tail & ~(0xffull << (8 * i))) | (b << (8 * i));
      }
    }
  }
  k.klen = klen;
}

enum : int { kCmpBad = 2 };
// Compare(key, target): bytewise (util/comparator.cc) or InternalKeyComparator
// (common/dbformat.cc:50-66); kCmpBad for an internal key shorter than 8 bytes.
__device__ __forceinline__ int compare(const KeyState& k, gcu8 t, uint64_t tlen, bool internal) {
  if (!internal) {
    const uint64_t m = k.klen < tlen ? k.klen : tlen;
    if (k.lcp < m) return k.sgn;
    return k.klen < tlen ? -1 : (k.klen > tlen ? 1 : 0);
  }
  if (k.klen < 8 || tlen < 8) return kCmpBad;
  const uint64_t uk = k.klen - 8, ut = tlen - 8, m = uk < ut ? uk : ut;
  if (k.lcp < m) return k.sgn;
  if (uk != ut) return uk < ut ? -1 : 1;
  uint64_t tt = 0;
  for (uint32_t i = 0; i < 8; i++) tt |= (uint64_t)t[ut + i] << (8 * i);
  return k.tail > tt ? -1 : (k.tail < tt ? 1 : 0);
}

// GetVarint64 (util/coding.cc): at most 10 bytes, never past limit.
__device__ __forceinline__ bool varint64(gcu8 d, uint32_t& p, uint32_t limit, uint64_t& v) {
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

__global__ __launch_bounds__(kBlockThreads) void block_seek_kernel(BlockSeekArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const bool internal = a.cmp != 0;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.n; q += stride) {
    const uint64_t off = a.handles[2 * q], size64 = a.handles[2 * q + 1];
    uint32_t state = kSeekNotValid;
    uint64_t pos = 0, key_len = 0, voff = 0, vlen = 0, h0 = 0, h1 = 0;
    if (off > a.image_size || size64 > a.image_size - off || size64 > 0xffffffffull || size64 < 4) {
      state = kSeekBadContents;
    } else {
      const gcu8 d = gptr(a.image, off);
      const uint32_t size = (uint32_t)size64;
      const uint32_t nr = le32(d, size - 4);
      if (nr > (size - 4) / 4) {
        state = kSeekBadContents;
      } else if (nr == 0) {
        pos = size - 4;  // the empty iterator
      } else {
        const uint32_t restarts = size - (1 + nr) * 4;
        const uint64_t t0 = a.key_offsets[q], t1 = a.key_offsets[q + 1];
        const uint64_t tlen = t1 >= t0 ? t1 - t0 : 0;
        const gcu8 t = gptr(a.keys, t0);
        // the found-key window
        uint64_t fo = 0, fcap = 0;
        if (a.found) {
          const uint64_t f0 = a.found_offsets[q], f1 = a.found_offsets[q + 1];
          if (f0 <= f1 && f1 <= a.found_cap) {
            fo = f0;
            fcap = f1 - f0;
          }
        }
        const gu8 fw = gwptr(a.found, fo);
        bool bad = false;
        // binary search over the restart points (table/block.cc:226-250)
        uint32_t left = 0, right = nr - 1;
        while (left < right) {
          const uint32_t mid = (uint32_t)(((uint64_t)left + right + 1) / 2);
          Hdr h;
          if (!decode_entry(d, le32(d, restarts + 4u * mid), restarts, h) || h.shared != 0) {
            bad = true;
            break;
          }
          KeyState k = {0, 0, 0, 0};
          advance(k, d, h, t, tlen, internal);
          const int c = compare(k, t, tlen, internal);
          if (c == kCmpBad) {
            bad = true;
            break;
          }
          if (c < 0) left = mid;
          else right = mid - 1;
        }
        pos = restarts;
        // linear search from restart point `left` (:253-264)
        if (!bad) {
          uint32_t p = le32(d, restarts + 4u * left);
          KeyState k = {0, 0, 0, 0};
          while (p < restarts) {
            Hdr h;
            if (!decode_entry(d, p, restarts, h) || k.klen < h.shared) {
              bad = true;
              break;
            }
            advance(k, d, h, t, tlen, internal);
            for (uint32_t i = 0; i < h.ns; i++)  // the key so far, in place (clipped to the window)
              if ((uint64_t)h.shared + i < fcap) fw[(uint64_t)h.shared + i] = d[h.kp + i];
            const int c = compare(k, t, tlen, internal);
            if (c == kCmpBad) {
              bad = true;
              break;
            }
            if (c >= 0) {
              state = kSeekValid;
              pos = p;
              key_len = k.klen;
              voff = off + h.kp + h.ns;
              vlen = h.vl;
              if (a.flags & 1u) {  // BlockHandle::DecodeFrom (table/format.cc:23-30)
                uint32_t vp = h.kp + h.ns;
                const uint32_t vend = vp + h.vl;
                if (!varint64(d, vp, vend, h0) || !varint64(d, vp, vend, h1)) {
                  state = kSeekBadHandle;
                  h0 = h1 = 0;
                }
              }
              break;
            }
            p = h.kp + h.ns + h.vl;
          }
        }
        if (bad) state = kSeekBadEntry;  // CorruptionError (:280-286)
      }
    }
    a.state[q] = state;
    a.pos[q] = pos;
    a.key_len[q] = key_len;
    a.value[2 * q] = voff;
    a.value[2 * q + 1] = vlen;
    if (a.handle_out) {
      a.handle_out[2 * q] = h0;
      a.handle_out[2 * q + 1] = h1;
    }
  }
}

}  // namespace

// ---- host-callable launchers (used by block_engine.cc) ----
hipError_t launch_block_walk(const BlockWalkArgs& a, bool decode, int grid, hipStream_t stream) {
  if (decode)
    hipLaunchKernelGGL(block_walk_kernel<true>, dim3(grid), dim3(kBlockThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(block_walk_kernel<false>, dim3(grid), dim3(kBlockThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_block_seek(const BlockSeekArgs& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(block_seek_kernel, dim3(grid), dim3(kBlockThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
