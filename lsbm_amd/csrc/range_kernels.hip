// range_kernels.hip -- gfx950 kernels of LSbM's range query over the buffered
// tree (include/lsbm_range.h): the file plan of Version::RangeQuery
// (lsbm/version_set.cc:1043-1214) and the count of Table::InternalGetRange
// (table/table.cc:340-368) over the range index.
//
// range_check_kernel        one lane per slot, run entry, bound, cursor offset
//                           and query: the slot table is sorted, the run and
//                           offset lists do not decrease and stay inside their
//                           buffers, the keys are long enough.
// range_plan_kernel         one lane per query: the number of files it reads.
// range_first_check_kernel  one lane per query: d_pair_first steps by the
//                           counts and ends inside pair_cap.
// range_emit_kernel         one lane per query: its files, in read order.
// range_index_check_kernel  one lane per index entry, file, query and pair.
// range_count_kernel        one wave per (query, file) pair: the Seek and the
//                           count up to the end key.
// range_reduce_kernel       one lane per query: found and total.
//
// The plan is a walk over sorted-table metadata: per slot a binary search over
// the files' largest keys and a few compares with their bounds.  The slot
// table, the run list, the use lengths and the cursor offsets are the same for
// every lane.  A level's slots are passed twice by the emit kernel (what the
// covered flags say, then the files they let through); the second pass hits
// the cache.
//
// The count kernel's wave finds the Seek position with a 64-way search (each
// lane one pivot, a ballot picks the interval: 3 steps for 100,000 entries),
// then steps 64 entries at a time: the lanes read 64 consecutive offsets and
// the keys between them, which lie side by side in the arena, compare each
// whole internal key bytewise with the end lookup key, and a ballot finds the
// first lane whose entry is past it.  The stop predicate is not monotone in
// the table's order, so nothing is searched for.  Every ballot is executed by
// all 64 lanes: the loops' trip counts depend only on wave-uniform values.
//
// Every kernel that reads a key runs after the check kernel of its call on the
// same stream and leaves at once when it set the status word, so bytes are
// addressed only through offsets that were checked, and the emit kernel stores
// only inside [pair_first[q], pair_first[q + 1]), which the first-check kernel
// has placed inside pair_cap.  Every loop advances.  No LDS, no spin-waits, no
// cross-workgroup state; the status word's atomicMax in the check kernels is
// the only atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"       // gcu8, gptr, load8, global_index
#include "key_compare_device.h"  // bytes_compare, internal_compare
#include "range_types.h"

namespace lsbm {
namespace {

__device__ __forceinline__ bool bad_keys(const RangeKeys& k, uint64_t i) {
  const uint64_t slo = k.start_offsets[i], shi = k.start_offsets[i + 1];
  const uint64_t elo = k.end_offsets[i], ehi = k.end_offsets[i + 1];
  return slo > shi || shi > k.start_size || shi - slo < 16 || elo > ehi || ehi > k.end_size || ehi - elo < 16;
}

__global__ __launch_bounds__(kRangeThreads) void range_check_kernel(RangePlanArgs a) {
  const uint64_t i = global_index<kRangeThreads>();
  bool bad = false;
  if (i < a.n_slots) {
    const uint32_t info = a.slot_info[i], kind = info & 0xff, level = (info >> 8) & 0xff, key = info & 0xffff;
    bad = level >= kRangeLevels || kind > kRsIns || (info >> 16) > (kRangeCovers | kRangeSole) ||
          ((level == 0) != (kind <= kRsL0Ins));
    if (i > 0) {
      const uint32_t prev = a.slot_info[i - 1] & 0xffff;
      // (kind | level << 8 is the sort key itself)
      bad = bad || key < prev || (key == prev && kind != kRsWb && kind != kRsCb);
    }
    bad = bad || a.run_first[i] > a.run_first[i + 1];
  }
  if (i == 0) bad = bad || a.run_first[0] != 0 || a.run_first[a.n_slots] != a.n_runs;
  if (i < 2 * a.n_runs) {
    const uint64_t lo = a.bound_offsets[i], hi = a.bound_offsets[i + 1];
    bad = bad || lo > hi || hi > a.bounds_size || hi - lo < 8;
  }
  if (i < kRangeCursors) {
    const uint64_t lo = a.cursor_offsets[i], hi = a.cursor_offsets[i + 1];
    bad = bad || lo > hi || hi > a.cursor_size;
  }
  if (i < a.q.n) bad = bad || bad_keys(a.q, i);
  if (bad) atomicMax(a.status, kRangeBadInput);
}

struct Query {
  gcu8 start, end;       // the user keys
  uint64_t slen, elen;   // their lengths
  gcu8 find;             // the start user key read as an internal key (FindFile's quirk):
  uint64_t flen, ftag;   // its "user key" and its "tag"
};

// One slot's walk: the files it pushes.  With `emit` they go to pair at...
__device__ uint32_t walk_slot(const RangePlanArgs& a, uint64_t s, bool find, const Query& k, bool emit, uint64_t at,
                              uint32_t flags) {
  const uint64_t lo = a.run_first[s], hi = a.run_first[s + 1];
  uint64_t i = lo;
  if (find) {  // FindFile (:130-150): the first file whose largest key is not below the key
    uint64_t left = lo, right = hi;
    while (left < right) {
      const uint64_t mid = left + (right - left) / 2;
      const uint64_t b = a.bound_offsets[2 * mid + 1], e = a.bound_offsets[2 * mid + 2];
      if (internal_compare(a.bounds, b, e - b, k.find, k.flen, k.ftag) < 0) {
        left = mid + 1;
      } else {
        right = mid;
      }
    }
    i = right;
  }
  uint32_t hits = 0;
  for (; i < hi; i++) {
    const uint64_t b0 = a.bound_offsets[2 * i], b1 = a.bound_offsets[2 * i + 1], b2 = a.bound_offsets[2 * i + 2];
    const int c = bytes_compare(k.end, k.elen, gptr(a.bounds, b0), b1 - b0 - 8);
    if (c >= 0 && bytes_compare(k.start, k.slen, gptr(a.bounds, b1), b2 - b1 - 8) <= 0) {
      if (emit) {
        a.pair_run[at + hits] = (uint32_t)i;
        a.pair_flags[at + hits] = flags;
      }
      hits++;
    }
    if (find && c < 0) break;
  }
  return hits;
}

// The files of query q; with kEmit they go to the pairs at...
template <bool kEmit>
__device__ __forceinline__ uint32_t range_walk(const RangePlanArgs& a, uint64_t q, uint64_t at) {
  const uint64_t n_slots = a.n_slots;
  Query k;
  const uint64_t so = a.q.start_offsets[q], eo = a.q.end_offsets[q];
  k.start = gptr(a.q.start_keys, so);
  k.slen = a.q.start_offsets[q + 1] - so - 8;
  k.end = gptr(a.q.end_keys, eo);
  k.elen = a.q.end_offsets[q + 1] - eo - 8;
  k.find = k.start;
  k.flen = k.slen - 8;  // (the check kernel: a user key of 8 bytes at least)
  k.ftag = load8(k.start + k.flen);
  uint32_t count = 0;
  uint64_t s = 0;
  // Level 0 (:1060-1077): every overlapping file of the deletion table, then the insertion table's walk
  for (; s < n_slots && ((a.slot_info[s] >> 8) & 0xff) == 0; s++)
    count += walk_slot(a, s, (a.slot_info[s] & 0xff) != kRsAll, k, kEmit, at + count, 0);
  const uint64_t uo = a.cursor_offsets[kRangeLevels], ul = a.cursor_offsets[kRangeLevels + 1] - uo;
  const bool below_upto = bytes_compare(k.end, k.elen, gptr(a.cursor_keys, uo), ul) < 0;
  for (uint32_t level = 1; level < kRangeLevels; level++) {
    uint64_t e = s;
    while (e < n_slots && ((a.slot_info[e] >> 8) & 0xff) == level) e++;
    const uint32_t use = a.use_len[level], use_wb = a.use_len[level - 1];
    bool checkwb = false;
    if (a.wb_enabled[level]) {
      const uint64_t co = a.cursor_offsets[level], cl = a.cursor_offsets[level + 1] - co;
      checkwb = bytes_compare(k.start, k.slen, gptr(a.cursor_keys, co), cl) > 0;
    }
    const bool cb_gate = use > 0 && below_upto;
    uint32_t n_wb = 0, n_del = 0, n_cb = 0, n_ins = 0, emitted = 0;
    bool wb_covered = false, cb_covered = false;
    // pass 0: what the walks push, and the covered flags; pass 1: the files the flags keep, in order
    for (uint32_t pass = 0; pass < (kEmit ? 2u : 1u); pass++) {
      uint32_t jw = 0, jc = 0;
      for (uint64_t t = s; t < e; t++) {
        const uint32_t info = a.slot_info[t], kind = info & 0xff;
        const bool covers = (info >> 16) & kRangeCovers, sole = (info >> 16) & kRangeSole;
        bool take;
        if (kind == kRsWb) {  // :1096-1124, from the head itself, tablecount++ > use_len[L-1] first
          take = checkwb && jw <= use_wb && (pass == 0 || wb_covered);
          jw++;
        } else if (kind == kRsDel) {  // :1132-1145
          take = !wb_covered;
        } else if (kind == kRsCb) {  // :1147-1178
          const bool skip = wb_covered || n_del > 0;
          const bool visit = skip ? (sole ? use >= 2 : (jc >= 1 && jc < use)) : jc < use;
          take = cb_gate && visit && (pass == 0 || cb_covered);
          jc++;
        } else {  // :1187-1198
          take = !cb_covered;
        }
        if (!take) continue;
        const uint32_t h = walk_slot(a, t, true, k, pass == 1, at + count + emitted, level << 8);
        if (pass == 1) {
          emitted += h;
        } else if (kind == kRsWb) {
          n_wb += h;
          wb_covered = wb_covered || (h > 0 && covers);
        } else if (kind == kRsDel) {
          n_del += h;
        } else if (kind == kRsCb) {
          n_cb += h;
          cb_covered = cb_covered || (h > 0 && covers);
        } else {
          n_ins += h;
        }
      }
    }
    const uint32_t read = (wb_covered ? n_wb : n_del) + (cb_covered ? n_cb : n_ins);
    // levelfound is overwritten by every file of tmp (:1202-1207): the last one is the level's answer; level 0's
    // files are still in tmp when level 1 is read
    const uint32_t group = read + (level == 1 ? count : 0);
    count += read;
    if (kEmit && group > 0) a.pair_flags[at + count - 1] = ((read > 0 ? level : 0u) << 8) | kRangeLast;
    s = e;
  }
  return count;
}

__global__ __launch_bounds__(kRangeThreads) void range_plan_kernel(RangePlanArgs a) {
  const uint64_t q = global_index<kRangeThreads>();
  if (q >= a.q.n || *a.status) return;
  a.count[q] = range_walk<false>(a, q, 0);
}

__global__ __launch_bounds__(kRangeThreads) void range_first_check_kernel(RangePlanArgs a) {
  const uint64_t q = global_index<kRangeThreads>();
  if (q > a.q.n || *a.status) return;
  if (q == a.q.n) {
    if (a.pair_first[q] > a.pair_cap) atomicMax(a.status, kRangeNoRoom);
    return;
  }
  const uint64_t lo = a.pair_first[q], hi = a.pair_first[q + 1];
  if (lo > hi || hi - lo != range_walk<false>(a, q, 0)) atomicMax(a.status, kRangeBadInput);
}

__global__ __launch_bounds__(kRangeThreads) void range_emit_kernel(RangePlanArgs a) {
  const uint64_t q = global_index<kRangeThreads>();
  if (q >= a.q.n || *a.status) return;
  a.checked[q] = range_walk<true>(a, q, a.pair_first[q]);
}

// ---------------------------------------------------------------- the count

__global__ __launch_bounds__(kRangeThreads) void range_index_check_kernel(RangeCountArgs a) {
  const uint64_t i = global_index<kRangeThreads>();
  bool bad = false;
  if (i < a.n_entries) {
    const uint64_t lo = a.index_offsets[i], hi = a.index_offsets[i + 1];
    bad = lo > hi || hi > a.index_size || hi - lo < 8;
  }
  if (i < a.n_files) bad = bad || a.file_first[i] > a.file_first[i + 1];
  if (i == 0) bad = bad || a.file_first[a.n_files] > a.n_entries || a.pair_first[0] != 0 || a.pair_first[a.q.n] != a.n_pairs;
  if (i < a.q.n) bad = bad || bad_keys(a.q, i) || a.pair_first[i] > a.pair_first[i + 1];
  if (i < a.n_pairs) bad = bad || a.pair_file[i] >= a.n_files;
  if (bad) atomicMax(a.status, kRangeBadInput);
}

__global__ __launch_bounds__(kRangeThreads) void range_count_kernel(RangeCountArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t p = (uint64_t)blockIdx.x * (kRangeThreads / 64) + (threadIdx.x >> 6);
  if (p >= a.n_pairs || *a.status) return;
  // the pair's query: the last q with pair_first[q] <= p (pair_first[0] = 0, pair_first[n] = n_pairs > p)
  uint64_t lo = 0, hi = a.q.n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.pair_first[mid] <= p) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  const uint64_t q = lo - 1;
  const uint32_t f = a.pair_file[p];
  if (a.file_state[f]) {  // a file that does not open for iteration: 0, and the flag
    if (lane == 0) {
      a.pair_count[p] = 0;
      a.pair_error[p] = 1;
    }
    return;
  }
  const uint64_t first = a.file_first[f], last = a.file_first[f + 1];
  const uint64_t so = a.q.start_offsets[q], ulen = a.q.start_offsets[q + 1] - so - 8;
  const gcu8 su = gptr(a.q.start_keys, so);
  const uint64_t stag = load8(su + ulen);
  const uint64_t eo = a.q.end_offsets[q], elen = a.q.end_offsets[q + 1] - eo;
  const gcu8 ek = gptr(a.q.end_keys, eo);
  // iter->Seek(start): the lower bound under the internal comparator, 64 pivots a step.  The answer is in [lo, hi].
  lo = first;
  hi = last;
  while (lo < hi) {
    const uint64_t step = (hi - lo + 63) >> 6, idx = lo + lane * step;
    bool below = false;
    if (idx < hi) {
      const uint64_t ko = a.index_offsets[idx];
      below = internal_compare(a.index_keys, ko, a.index_offsets[idx + 1] - ko, su, ulen, stag) < 0;
    }
    const uint64_t mask = __ballot(below);
    const uint32_t k = mask == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~mask);  // the pivots below: a prefix
    if (k == 0) {
      hi = lo;
    } else {
      const uint64_t next = lo + k * step;
      lo = lo + (k - 1) * step + 1;  // (pivot k - 1 is inside [lo, hi): its lane saw idx < hi)
      hi = next < hi ? next : hi;
    }
  }
  const uint64_t seek = lo;
  // count up to the first entry whose whole internal key is bytewise past the whole end lookup key
  uint64_t pos = seek, count;
  for (;;) {
    const uint64_t idx = pos + lane;
    bool stop = false;
    if (idx < last) {
      const uint64_t ko = a.index_offsets[idx];
      stop = bytes_compare(gptr(a.index_keys, ko), a.index_offsets[idx + 1] - ko, ek, elen) > 0;
    }
    const uint64_t mask = __ballot(stop);
    if (mask) {
      count = pos + (uint32_t)__builtin_ctzll(mask) - seek;
      break;
    }
    pos += 64;
    if (pos >= last) {
      count = last - seek;
      break;
    }
  }
  if (lane == 0) {
    a.pair_count[p] = (uint32_t)count;
    a.pair_error[p] = 0;
  }
}

__global__ __launch_bounds__(kRangeThreads) void range_reduce_kernel(RangeCountArgs a) {
  const uint64_t q = global_index<kRangeThreads>();
  if (q >= a.q.n || *a.status) return;
  uint32_t found = 0;
  uint64_t total = 0;
  for (uint64_t p = a.pair_first[q]; p < a.pair_first[q + 1]; p++) {
    const uint32_t c = a.pair_count[p];
    total += c;
    if (a.pair_flags[p] & kRangeLast) found += c;
  }
  a.found[q] = found;
  a.total[q] = total;
}

uint32_t groups(uint64_t n) { return (uint32_t)((n + kRangeThreads - 1) / kRangeThreads); }

hipError_t launch_checks(const RangePlanArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  uint64_t items = a.n_slots > a.q.n ? a.n_slots : a.q.n;
  if (items < 2 * a.n_runs) items = 2 * a.n_runs;
  if (items < kRangeCursors) items = kRangeCursors;
  hipLaunchKernelGGL(range_check_kernel, dim3(groups(items)), dim3(kRangeThreads), 0, stream, a);
  return hipSuccess;
}

}  // namespace

hipError_t launch_range_plan(const RangePlanArgs& a, hipStream_t stream) {
  const hipError_t e = launch_checks(a, stream);
  if (e != hipSuccess) return e;
  if (a.q.n) hipLaunchKernelGGL(range_plan_kernel, dim3(groups(a.q.n)), dim3(kRangeThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_range_emit(const RangePlanArgs& a, hipStream_t stream) {
  const hipError_t e = launch_checks(a, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(range_first_check_kernel, dim3(groups(a.q.n + 1)), dim3(kRangeThreads), 0, stream, a);
  if (a.q.n) hipLaunchKernelGGL(range_emit_kernel, dim3(groups(a.q.n)), dim3(kRangeThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_range_count(const RangeCountArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  uint64_t items = a.n_entries > a.n_pairs ? a.n_entries : a.n_pairs;
  if (items < a.n_files) items = a.n_files;
  if (items < a.q.n) items = a.q.n;
  if (items < 1) items = 1;
  hipLaunchKernelGGL(range_index_check_kernel, dim3(groups(items)), dim3(kRangeThreads), 0, stream, a);
  if (a.n_pairs)
    hipLaunchKernelGGL(range_count_kernel, dim3((uint32_t)((a.n_pairs + kRangeThreads / 64 - 1) / (kRangeThreads / 64))),
                       dim3(kRangeThreads), 0, stream, a);
  if (a.q.n) hipLaunchKernelGGL(range_reduce_kernel, dim3(groups(a.q.n)), dim3(kRangeThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
