// iter_kernels.hip -- gfx950 kernels of the batched range scan
// (include/lsbm_iter.h): DBIter of lsbm/db_iter.cc over merged entries at a
// snapshot, for many range queries at once.
//
// iter_offsets_kernel  one lane per item of an offsets array: it does not
//                      decrease, stays inside its buffer and has the bytes the
//                      caller needs; else the status word is set.
// iter_check_kernel    one lane per entry: its key's offsets and length, and
//                      Compare(key e, key e+1) <= 0.
// iter_flag_kernel     one lane per merged position: visible / corrupt /
//                      seg_start / value from its tag and its predecessor's
//                      user key, kept as a byte; per tile the last seg_start
//                      and the last visible position, the corrupt entries, the
//                      yields that are certain, and the one entry whose head
//                      flag hangs on the tiles before (below).
// iter_scan_kernel     one workgroup: running maxima and sums over the tiles,
//                      the counts and the slots after the last entry.
// iter_emit_kernel     one lane per merged position: redoes the in-tile scans
//                      on the flag bytes -> live, the ranks, first, back.
// iter_range_kernel    one lane per query: two lower bounds over the entries,
//                      then the query's window of live entries, its status and
//                      its output bytes.
// iter_emit_out_kernel one wave per 64 output entries: each lane places its
//                      entry, then all 64 lanes copy the wave's user-key bytes
//                      and then its value bytes as flat byte ranges, 8 bytes a
//                      lane, finding each chunk's entry in the wave's LDS row.
//
// head(p) = visible(p) && B(p) < A(p), with A(p) the last seg_start position at
// or before p and B(p) the last visible position before p (both max-scans,
// kept as position + 1 so that 0 is "none").  Inside a tile both are known
// except for entries before the tile's first seg_start, which continue the
// user key of the tile before: there an entry with a visible one before it in
// the tile is hidden for certain, and only the tile's first visible entry can
// be a head -- if no entry of its user key is visible in the tiles before.
// That one candidate per tile is settled by the scan kernel, so the entries
// are read twice and no workgroup waits for another.
//
// Every kernel that reads key bytes runs after the check kernels of its call
// on the same stream and leaves at once when they set the status word, so key
// bytes are addressed only through offsets that were checked; indices read
// back from scratch or from the caller (the view, the queries' windows) are
// checked against their limits before they address anything.  Every loop halves
// a range or advances.  No spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // gcu8, gu8, gptr, gwptr, load8, store8, wave_phase, wave_incl_scan, global_index
#include "iter_types.h"
#include "key_compare_device.h"  // bytes_compare, internal_compare

namespace lsbm {
namespace {

constexpr uint32_t kTypeValue = 1;  // common/dbformat.h; kValueTypeForSeek is the same

__device__ __forceinline__ uint64_t wave_incl_max(uint64_t v, uint32_t lane) {
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(v, o);
    if (lane >= o && t > v) v = t;
  }
  return v;
}

// exclusive sums of x[0..2] over the workgroup's lanes in lane order, and the totals
__device__ __forceinline__ void block_excl_sum3(const uint64_t (&x)[3], uint64_t (*lds)[3], uint64_t (&ex)[3],
                                                uint64_t (&tot)[3]) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc[3];
  for (int k = 0; k < 3; k++) {
    inc[k] = wave_incl_scan(x[k], lane);
    if (lane == 63) lds[w][k] = inc[k];
  }
  __syncthreads();
  for (int k = 0; k < 3; k++) {
    uint64_t before = 0, all = 0;
    for (uint32_t i = 0; i < (uint32_t)kIterWaves; i++) {
      if (i < w) before += lds[i][k];
      all += lds[i][k];
    }
    ex[k] = before + inc[k] - x[k];
    tot[k] = all;
  }
  __syncthreads();  // (the rows are free for the caller's next round)
}

// running maxima of a and of b over the lanes before each lane, in lane
// order, and over all lanes
__device__ __forceinline__ void block_max2(uint64_t a, uint64_t b, uint64_t (*lds)[3], uint64_t& before_a,
                                           uint64_t& before_b, uint64_t& all_a, uint64_t& all_b) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t ia = wave_incl_max(a, lane), ib = wave_incl_max(b, lane);
  uint64_t ea = __shfl_up(ia, 1), eb = __shfl_up(ib, 1);
  if (lane == 0) ea = eb = 0;
  if (lane == 63) {
    lds[w][0] = ia;
    lds[w][1] = ib;
  }
  __syncthreads();
  uint64_t oa = 0, ob = 0;
  all_a = 0;
  all_b = 0;
  for (uint32_t i = 0; i < (uint32_t)kIterWaves; i++) {
    const uint64_t xa = lds[i][0], xb = lds[i][1];
    if (i < w) {
      oa = xa > oa ? xa : oa;
      ob = xb > ob ? xb : ob;
    }
    all_a = xa > all_a ? xa : all_a;
    all_b = xb > all_b ? xb : all_b;
  }
  __syncthreads();  // (the rows are free for the caller's next round)
  before_a = ea > oa ? ea : oa;
  before_b = eb > ob ? eb : ob;
}

__global__ __launch_bounds__(kIterThreads) void iter_offsets_kernel(IterOffsetsArgs a) {
  const uint64_t i = global_index<kIterThreads>();
  if (i >= a.n) return;
  const uint64_t lo = a.offsets[i], hi = a.offsets[i + 1];
  if (lo > hi || hi > a.size || hi - lo < a.min_len) atomicMax(a.status, kIterBadInput);
}

// ---------------------------------------------------------------- plan

__device__ __forceinline__ bool key_ok(const IterEntries& e, uint64_t ka, uint64_t kb) {
  return ka <= kb && kb <= e.keys_size && kb - ka >= 8;
}

__global__ __launch_bounds__(kIterThreads) void iter_check_kernel(IterPlanArgs a) {
  const uint64_t e = global_index<kIterThreads>();
  if (e >= a.e.n) return;
  const uint64_t ka = a.e.key_offsets[e], kb = a.e.key_offsets[e + 1];
  uint32_t st = kIterOk;
  if (!key_ok(a.e, ka, kb)) {
    st = kIterBadInput;
  } else if (e + 1 < a.e.n) {
    const uint64_t nb = a.e.key_offsets[e + 2];
    if (key_ok(a.e, kb, nb)) {
      const gcu8 k = gptr(a.e.keys, ka), s = gptr(a.e.keys, kb);
      int c = bytes_compare(k, kb - ka - 8, s, nb - kb - 8);
      if (c == 0) {
        const uint64_t t = load8(k + (kb - ka - 8)), u = load8(s + (nb - kb - 8));
        c = t > u ? -1 : (t < u ? 1 : 0);  // (tag_compare, spelled out: it compiles differently here)
      }
      if (c > 0) st = kIterUnsorted;
    }
  }
  if (st != kIterOk) atomicMax(a.status, st);
}

// the in-tile scans over a position's flag byte: a_loc / b_loc are A / B as
// lane + 1 inside the tile, 0 where the tile does not say
__device__ __forceinline__ void tile_scans(uint32_t f, uint64_t (*lds)[3], uint64_t& a_loc, uint64_t& b_loc,
                                           uint64_t& all_a, uint64_t& all_b) {
  const uint64_t own = (f & kFlagSegStart) ? threadIdx.x + 1 : 0;
  block_max2(own, (f & kFlagVisible) ? threadIdx.x + 1 : 0, lds, a_loc, b_loc, all_a, all_b);
  if (own) a_loc = own;  // (A counts the position itself)
}

__global__ __launch_bounds__(kIterThreads) void iter_flag_kernel(IterPlanArgs a) {
  __shared__ uint64_t lds[kIterWaves][3];
  __shared__ uint64_t s_cand;
  if (*a.status) return;  // (uniform: set only by the kernels before)
  const uint64_t base = (uint64_t)blockIdx.x * kIterThreads, p = base + threadIdx.x;
  if (threadIdx.x == 0) s_cand = 0;
  uint32_t f = 0;
  uint64_t klen = 0;
  if (p < a.e.n) {
    const uint64_t ka = a.e.key_offsets[p];
    klen = a.e.key_offsets[p + 1] - ka;
    const gcu8 k = gptr(a.e.keys, ka);
    const uint64_t tag = load8(k + (klen - 8));
    const uint32_t type = (uint32_t)(tag & 0xff);
    if (type <= kTypeValue) {  // ParseInternalKey
      if ((tag >> 8) <= a.snapshot) f |= kFlagVisible;
      if (type == kTypeValue) f |= kFlagValue;
    } else {
      f |= kFlagCorrupt;
    }
    bool seg = p == 0;
    if (!seg) {
      const uint64_t pa = a.e.key_offsets[p - 1];
      seg = bytes_compare(gptr(a.e.keys, pa), ka - pa - 8, k, klen - 8) != 0;
    }
    if (seg) f |= kFlagSegStart;
    a.flags[p] = (uint8_t)f;
  }
  uint64_t a_loc, b_loc, all_a, all_b;
  tile_scans(f, lds, a_loc, b_loc, all_a, all_b);
  const bool visible = (f & kFlagVisible) != 0, value = (f & kFlagValue) != 0;
  // with a seg_start in the tile at or before p the tile decides; without one, only the first visible entry is open
  const bool yields = visible && value && a_loc != 0 && b_loc < a_loc;
  if (visible && value && a_loc == 0 && b_loc == 0) s_cand = (klen << 1) | 1u;  // (one lane at most)
  const uint64_t x[3] = {yields ? 1u : 0u, yields ? klen : 0, (f & kFlagCorrupt) ? 1u : 0u};
  uint64_t ex[3], tot[3];
  block_excl_sum3(x, lds, ex, tot);  // (its barriers order s_cand)
  if (threadIdx.x == 0) {
    uint64_t* t = a.tiles + kIterTileWords * (uint64_t)blockIdx.x;
    t[0] = all_a ? base + all_a : 0;
    t[1] = all_b ? base + all_b : 0;
    t[2] = tot[2];
    t[3] = tot[0];
    t[4] = tot[1];
    t[5] = s_cand;
  }
}

// one value's running maximum (kMax) or sum over the lanes before each lane, and over all lanes
template <bool kMax>
__device__ __forceinline__ void block_excl1(uint64_t x, uint64_t* lds, uint64_t& before, uint64_t& all) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t inc = kMax ? wave_incl_max(x, lane) : wave_incl_scan(x, lane);
  uint64_t ex = __shfl_up(inc, 1);
  if (lane == 0) ex = 0;
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  uint64_t o = 0;
  all = 0;
  for (uint32_t i = 0; i < (uint32_t)kIterWaves; i++) {
    const uint64_t v = lds[i];
    if (i < w) o = kMax ? (v > o ? v : o) : o + v;
    all = kMax ? (v > all ? v : all) : all + v;
  }
  __syncthreads();
  before = kMax ? (ex > o ? ex : o) : ex + o;
}

__global__ __launch_bounds__(kIterThreads) void iter_scan_kernel(IterPlanArgs a) {
  __shared__ uint64_t lds[kIterWaves];
  __shared__ uint64_t s_carry[6];  // A, B, then the sums: yields, their key bytes, corrupt entries; one to pad
  if (*a.status) return;
  if (threadIdx.x < 5) s_carry[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t base = 0; base < a.n_tiles; base += kIterThreads) {
    const uint64_t t = base + threadIdx.x;
    uint64_t* w = a.tiles + kIterTileWords * t;
    const bool in = t < a.n_tiles;
    // A and B before the tile: the maxima over the tiles before it (each result is stored before the next
    // scan starts: five scans' worth of live values pass 64 registers)
    uint64_t in_a, in_b, all_a, all_b;
    block_excl1<true>(in ? w[0] : 0, lds, in_a, all_a);
    block_excl1<true>(in ? w[1] : 0, lds, in_b, all_b);
    in_a = s_carry[0] > in_a ? s_carry[0] : in_a;
    in_b = s_carry[1] > in_b ? s_carry[1] : in_b;
    const uint64_t cand = in ? w[5] : 0;
    const bool head = (cand & 1) && in_b < in_a;  // no visible entry of the candidate's user key before the tile
    if (in) {
      w[0] = in_a;
      w[1] = in_b;
    }
    uint64_t ex, ty, tb, tc;
    block_excl1<false>((in ? w[3] : 0) + (head ? 1 : 0), lds, ex, ty);
    if (in) w[3] = s_carry[2] + ex;
    block_excl1<false>((in ? w[4] : 0) + (head ? cand >> 1 : 0), lds, ex, tb);
    if (in) w[4] = s_carry[3] + ex;
    block_excl1<false>(in ? w[2] : 0, lds, ex, tc);
    if (in) w[2] = s_carry[4] + ex;
    __syncthreads();  // (every lane has read the carries)
    if (threadIdx.x == 0) {
      s_carry[0] = all_a > s_carry[0] ? all_a : s_carry[0];
      s_carry[1] = all_b > s_carry[1] ? all_b : s_carry[1];
      s_carry[2] += ty;
      s_carry[3] += tb;
      s_carry[4] += tc;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint64_t ny = s_carry[2], bytes = s_carry[3];
    if (ny > a.e.n) ny = bytes = 0;  // (cannot be: the slot below stays inside n + 1)
    a.counts[0] = ny;
    a.counts[1] = bytes;
    a.counts[2] = s_carry[4];
    a.out_key_offsets[ny] = bytes;  // the slot after the last live entry
    a.yield_rank[a.e.n] = ny;
    a.corrupt_rank[a.e.n] = s_carry[4];
  }
}

__global__ __launch_bounds__(kIterThreads) void iter_emit_kernel(IterPlanArgs a) {
  __shared__ uint64_t lds[kIterWaves][3];
  if (*a.status) return;
  const uint64_t base = (uint64_t)blockIdx.x * kIterThreads, p = base + threadIdx.x;
  const uint64_t* t = a.tiles + kIterTileWords * (uint64_t)blockIdx.x;
  uint32_t f = 0;
  uint64_t klen = 0;
  if (p < a.e.n) {
    f = a.flags[p];
    klen = a.e.key_offsets[p + 1] - a.e.key_offsets[p];
  }
  uint64_t a_loc, b_loc, all_a, all_b;
  tile_scans(f, lds, a_loc, b_loc, all_a, all_b);
  const uint64_t A = a_loc ? base + a_loc : t[0], B = b_loc ? base + b_loc : t[1];
  const bool yields = (f & kFlagVisible) && (f & kFlagValue) && B < A;
  const uint64_t x[3] = {yields ? 1u : 0u, yields ? klen : 0, (f & kFlagCorrupt) ? 1u : 0u};
  uint64_t ex[3], tot[3];
  block_excl_sum3(x, lds, ex, tot);
  if (p >= a.e.n) return;
  const uint64_t j = t[3] + ex[0];
  a.yield_rank[p] = j;
  a.corrupt_rank[p] = t[2] + ex[2];
  if (yields && j < a.e.n && A >= 1) {
    a.source[j] = p;
    a.out_key_offsets[j] = t[4] + ex[1];
    a.first[j] = A - 1;
    a.back[j] = (int64_t)B - 1;
  }
}

// ---------------------------------------------------------------- range

// the first entry that is not before the lookup key (u, tag): DBIter::Seek's iter_->Seek
__device__ __forceinline__ uint64_t seek_entries(const IterEntries& e, gcu8 u, uint64_t ulen, uint64_t tag) {
  uint64_t lo = 0, hi = e.n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t ea = e.key_offsets[mid], el = e.key_offsets[mid + 1] - ea;
    if (internal_compare(e.keys, ea, el, u, ulen, tag) < 0) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

__global__ __launch_bounds__(kIterThreads) void iter_range_kernel(IterRangeArgs a) {
  const uint64_t q = global_index<kIterThreads>();
  if (q >= a.n_queries || *a.status) return;
  const uint64_t n = a.e.n, ny = a.v.counts[0];
  const uint64_t tag = (a.snapshot << 8) | kTypeValue;
  uint64_t p_lo = 0, p_hi = n;
  const bool has_hi = a.hi_offsets && (!a.hi_present || a.hi_present[q]);
  if (!a.lo_present || a.lo_present[q]) {
    const uint64_t at = a.lo_offsets[q];
    p_lo = seek_entries(a.e, gptr(a.lo_keys, at), a.lo_offsets[q + 1] - at, tag);
  }
  if (has_hi) {
    const uint64_t at = a.hi_offsets[q];
    p_hi = seek_entries(a.e, gptr(a.hi_keys, at), a.hi_offsets[q + 1] - at, tag);
  }
  const uint64_t j_lo = a.v.yield_rank[p_lo], j_hi = a.v.yield_rank[p_hi];
  bool bad = ny > n || j_lo > ny || j_hi > ny;
  uint64_t limit = a.limits ? a.limits[q] : a.limit;
  if (limit > n) limit = n;  // (no query yields more)
  uint64_t jb = j_lo, cnt = 0;
  bool corrupt = false;
  if (!bad && limit > 0) {
    const uint64_t span = j_hi > j_lo ? j_hi - j_lo : 0;
    cnt = limit < span ? limit : span;
    if (!a.reverse) {
      // ParseKey runs on [p_lo, stop): up to the entry the iterator rests on, the one that fails key() < hi included
      uint64_t jl = j_lo + (limit - 1);
      if (jl > j_hi) jl = j_hi;
      if (jl < j_lo) jl = j_lo;
      uint64_t stop = n;
      if (jl < ny) {
        stop = a.v.live[jl];
        bad = stop >= n;
        stop += 1;
      }
      if (!bad && stop > p_lo) corrupt = a.v.corrupt_rank[stop] > a.v.corrupt_rank[p_lo];
    } else {
      jb = j_hi - cnt;
      uint64_t upper = n;
      if (has_hi && j_hi < ny) {  // Seek(hi) ends valid: parsed up to its entry, then Prev() steps over its user key
        const uint64_t at = a.v.live[j_hi];
        upper = a.v.first[j_hi];
        bad = at >= n || upper > at;
        if (!bad && at + 1 > p_hi) corrupt = a.v.corrupt_rank[at + 1] > a.v.corrupt_rank[p_hi];
      } else if (has_hi && p_hi < n) {  // Seek(hi) walks off the end, then SeekToLast()
        corrupt = a.v.corrupt_rank[n] > a.v.corrupt_rank[p_hi];
      }
      // the yield the iterator rests on at the end: the limit-th, or the one that fails key() >= lo
      int64_t jt = (int64_t)j_hi - (int64_t)limit;
      if (jt < (int64_t)j_lo - 1) jt = (int64_t)j_lo - 1;
      if (jt > (int64_t)j_hi - 1) jt = (int64_t)j_hi - 1;
      uint64_t lower = 0;
      if (!bad && jt >= 0) {
        const int64_t b = a.v.back[jt];
        bad = b >= (int64_t)n;
        if (b >= 0) lower = (uint64_t)b;
      }
      if (!bad && upper > lower) corrupt = corrupt || a.v.corrupt_rank[upper] > a.v.corrupt_rank[lower];
    }
  }
  uint64_t kbytes = 0, vbytes = 0;
  if (!bad && cnt) {
    const uint64_t k0 = a.v.live_key_offsets[jb], k1 = a.v.live_key_offsets[jb + cnt];
    const uint64_t v0 = a.v.value_prefix[jb], v1 = a.v.value_prefix[jb + cnt];
    bad = k1 < k0 || k1 - k0 < 8 * cnt || v1 < v0;
    kbytes = k1 - k0 - 8 * cnt;
    vbytes = v1 - v0;
  }
  if (bad) {  // the view is not a plan of these entries
    atomicMax(a.status, kIterBadInput);
    return;
  }
  a.j_begin[q] = jb;
  a.count[q] = cnt;
  a.scan_status[q] = corrupt ? kScanCorruption : kScanOk;
  a.key_bytes[q] = kbytes;
  a.value_bytes[q] = vbytes;
}

// ---------------------------------------------------------------- emit

// all 64 lanes copy the wave's output bytes [lo, hi) of dst, 8 bytes a lane:
// entry l < cnt owns output bytes [s_out[l], s_out[l + 1]) and reads them from
// src + s_src[l]
__device__ __forceinline__ void wave_flat_copy(uint8_t* dst, const uint8_t* src, const uint64_t* s_out,
                                               const uint64_t* s_src, uint32_t cnt, uint64_t lo, uint64_t hi,
                                               uint32_t lane) {
  // chunk c is output bytes [8c, 8c + 8) cut to [lo, hi): every byte has one lane
  for (uint64_t c = (lo >> 3) + lane; (c << 3) < hi; c += 64) {
    const uint64_t q0 = (c << 3) > lo ? (c << 3) : lo;
    const uint64_t q1 = (c << 3) + 8 < hi ? (c << 3) + 8 : hi;
    // the entry of byte q0: the last l < cnt with s_out[l] <= q0 (s_out[0] = lo <= q0)
    uint32_t l = 0, h = cnt;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (s_out[mid] <= q0) l = mid; else h = mid;
    }
    if (q1 - q0 == 8 && q1 <= s_out[l + 1]) {
      const uint64_t x = load8(gptr(src, s_src[l] + (q0 - s_out[l])));
      store8(gwptr(dst, q0), x);
    } else {
      for (uint64_t q = q0; q < q1; q++) {
        while (q >= s_out[l + 1]) l++;  // (q < hi = s_out[cnt]: stops at l < cnt)
        dst[q] = src[s_src[l] + (q - s_out[l])];
      }
    }
  }
}

__global__ __launch_bounds__(kIterThreads) void iter_emit_out_kernel(IterEmitArgs a) {
  __shared__ uint64_t s_out[kIterWaves][65];  // the wave's entries' first output bytes, then the range's end
  __shared__ uint64_t s_src[kIterWaves][64];  // and their bytes' places in the input
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (*a.status) return;  // (set by the check kernels; a wave's own finding below stops only that wave)
  const uint64_t total = a.entry_first[a.n_queries], key_total = a.key_first[a.n_queries],
                 value_total = a.value_first[a.n_queries];
  if (total > a.entries_cap || key_total > a.out_keys_cap || value_total > a.out_values_cap) {  // (uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(a.status, kIterNoRoom);
    return;
  }
  const uint64_t i0 = ((uint64_t)blockIdx.x * kIterWaves + w) * 64;
  if (i0 > total) return;  // (wave-uniform; the waves share no LDS row)
  const uint64_t i = i0 + lane;
  const uint32_t cnt = (uint32_t)(total - i0 < 64 ? total - i0 : 64);
  if (i == total) {
    a.out_key_offsets[i] = key_total;
    a.out_value_offsets[i] = value_total;
  }
  uint64_t ko = 0, ko1 = 0, vo = 0, vo1 = 0, ksrc = 0, vsrc = 0;
  bool bad = false;
  if (lane < cnt) {
    bad = a.n_queries == 0;
  }
  if (lane < cnt && !bad) {
    // the query of output entry i: the last q with entry_first[q] <= i (its window is not empty: i < total)
    uint64_t q = 0, h = a.n_queries;
    while (h - q > 1) {
      const uint64_t mid = q + ((h - q) >> 1);
      if (a.entry_first[mid] <= i) q = mid; else h = mid;
    }
    const uint64_t e0 = a.entry_first[q], e1 = a.entry_first[q + 1], jb = a.j_begin[q];
    bad = i < e0 || i >= e1 || jb > a.n_live || e1 - e0 > a.n_live - jb;
    if (!bad) {
      const uint64_t r = i - e0, c = e1 - e0;
      const uint64_t j = a.reverse ? jb + (c - 1 - r) : jb + r;
      const uint64_t ka = a.live_key_offsets[j], kb = a.live_key_offsets[j + 1];
      const uint64_t va = a.value_prefix[j], vb = a.value_prefix[j + 1];
      const uint64_t at = a.live_values[2 * j], len = a.live_values[2 * j + 1];
      // where the query's window starts (ascending) or ends (descending) in the live bytes
      const uint64_t edge = a.reverse ? jb + c : jb;
      const uint64_t kedge = a.live_key_offsets[edge], vedge = a.value_prefix[edge];
      bad = ka > kb || kb > a.live_keys_size || kb - ka < 8 || va > vb || vb - va != len || at > a.image_size ||
            len > a.image_size - at;
      if (!bad) {
        // user bytes before live entry j: live_key_offsets[j] - 8j
        if (a.reverse) {
          bad = kedge < kb || kedge - kb < 8 * (edge - j - 1) || vedge < vb;
          ko = a.key_first[q] + (kedge - kb - 8 * (edge - j - 1));
          vo = a.value_first[q] + (vedge - vb);
        } else {
          bad = ka < kedge || ka - kedge < 8 * (j - edge) || va < vedge;
          ko = a.key_first[q] + (ka - kedge - 8 * (j - edge));
          vo = a.value_first[q] + (va - vedge);
        }
        ko1 = ko + (kb - ka - 8);
        vo1 = vo + len;
        bad = bad || ko > ko1 || ko1 > a.key_first[q + 1] || a.key_first[q + 1] > key_total || vo > vo1 ||
              vo1 > a.value_first[q + 1] || a.value_first[q + 1] > value_total;
        ksrc = ka;
        vsrc = at;
      }
    }
    if (!bad) {
      a.out_key_offsets[i] = ko;
      a.out_value_offsets[i] = vo;
    }
  }
  // the wave's entries must tile its byte ranges: each starts where the one before ends
  const uint64_t prev_k = __shfl_up(ko1, 1), prev_v = __shfl_up(vo1, 1);
  if (lane > 0 && lane < cnt && (prev_k != ko || prev_v != vo)) bad = true;
  if (__ballot(bad) != 0) {  // not a view of these entries: no byte of the wave is moved
    if (lane == 0) atomicMax(a.status, kIterBadInput);
    return;
  }
  if (cnt == 0) return;
  {
    const uint64_t lo = __shfl(ko, 0), hi = __shfl(ko1, (int)cnt - 1);
    s_out[w][lane] = lane < cnt ? ko : hi;
    if (lane == 0) s_out[w][64] = hi;
    s_src[w][lane] = ksrc;
    wave_phase();
    wave_flat_copy(a.out_keys, a.live_keys, s_out[w], s_src[w], cnt, lo, hi, lane);
    wave_phase();
  }
  {
    const uint64_t lo = __shfl(vo, 0), hi = __shfl(vo1, (int)cnt - 1);
    s_out[w][lane] = lane < cnt ? vo : hi;
    if (lane == 0) s_out[w][64] = hi;
    s_src[w][lane] = vsrc;
    wave_phase();
    wave_flat_copy(a.out_values, a.image, s_out[w], s_src[w], cnt, lo, hi, lane);
  }
}

uint32_t groups(uint64_t n) { return (uint32_t)((n + kIterThreads - 1) / kIterThreads); }

void check_offsets(const uint64_t* offsets, uint64_t n, uint64_t size, uint64_t min_len, uint32_t* status,
                   hipStream_t stream) {
  if (!n) return;
  const IterOffsetsArgs c = {offsets, n, size, min_len, status};
  hipLaunchKernelGGL(iter_offsets_kernel, dim3(groups(n)), dim3(kIterThreads), 0, stream, c);
}

}  // namespace

hipError_t launch_dbiter_plan(const IterPlanArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  if (a.e.n) {
    const dim3 grid((uint32_t)a.n_tiles), block(kIterThreads);
    hipLaunchKernelGGL(iter_check_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(iter_flag_kernel, grid, block, 0, stream, a);
  }
  hipLaunchKernelGGL(iter_scan_kernel, dim3(1), dim3(kIterThreads), 0, stream, a);
  if (a.e.n) hipLaunchKernelGGL(iter_emit_kernel, dim3((uint32_t)a.n_tiles), dim3(kIterThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_dbiter_range(const IterRangeArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  check_offsets(a.e.key_offsets, a.e.n, a.e.keys_size, 8, a.status, stream);
  check_offsets(a.lo_offsets, a.n_queries, a.lo_size, 0, a.status, stream);
  if (a.hi_offsets) check_offsets(a.hi_offsets, a.n_queries, a.hi_size, 0, a.status, stream);
  if (a.n_queries) hipLaunchKernelGGL(iter_range_kernel, dim3(groups(a.n_queries)), dim3(kIterThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_dbiter_emit(const IterEmitArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  // the three prefix arrays do not decrease (their ends are held against the caps by the kernel)
  check_offsets(a.entry_first, a.n_queries, ~0ull, 0, a.status, stream);
  check_offsets(a.key_first, a.n_queries, ~0ull, 0, a.status, stream);
  check_offsets(a.value_first, a.n_queries, ~0ull, 0, a.status, stream);
  // one wave per 64 output entries, and the slot after the last one
  const uint64_t wgs = a.entries_cap / kIterThreads + 1;
  hipLaunchKernelGGL(iter_emit_out_kernel, dim3((uint32_t)wgs), dim3(kIterThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
