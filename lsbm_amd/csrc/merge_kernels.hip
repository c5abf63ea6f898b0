// merge_kernels.hip -- gfx950 kernels of the batched compaction merge
// (include/lsbm_merge.h): MergingIterator over sorted runs (table/merger.cc)
// and the drop rule of DoCompactionWork (lsbm/db_impl.cc:999-1032).
//
// merge_init_kernel    one wave: run_first tiles [0, n), per-run status, the
//                      error word and the counts start at zero.
// merge_check_kernel   one lane per entry: its key's offsets and length, and
//                      Compare(key e, key e+1) <= 0 inside its run.
// merge_sample_kernel  one lane per sample (every kMergeSample-th entry of a
//                      run): its bound in every other run, a binary search
//                      over the whole run each, kept in scratch.
// merge_rank_kernel    one lane per entry: its position in the stable merge by
//                      (key, run, position) -- its index in its own run, plus
//                      an upper bound in every earlier run and a lower bound in
//                      every later one, each a binary search between the
//                      bounds of the two samples around it -- and
//                      order[rank] = e straight away (the ranks are a
//                      permutation, so rank and scatter are one kernel).
// merge_flag_kernel    one lane per merged position: the drop rule from
//                      order[p-1], order[p]; per tile of kMergeThreads
//                      positions the kept entries and their key bytes.
// merge_scan_kernel    one workgroup: running sums over the tiles, the counts.
// merge_emit_kernel    one lane per merged position: a kept entry's output
//                      index and key-byte offset -> source, out_key_offsets.
// merge_gather_kernel  one wave per 64 output entries: each lane moves its
//                      entry's offset and value slice, then all 64 lanes copy
//                      the wave's key bytes as one flat byte range, 8 bytes a
//                      lane, finding each chunk's entry in the wave's LDS row.
//
// Every kernel after merge_check runs only when no run is in error, that is on
// key offsets and run bounds that were checked; indices read back from scratch
// or from the caller (order, source, the plan's offsets) are checked against
// their limits before they address anything.  Every loop halves a range or
// advances.  No spin-waits, no cross-workgroup state inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"       // gcu8, gptr, gwptr, load8, store8, wave_phase, wave_incl_scan
#include "key_compare_device.h"  // bytes_compare, tag_compare
#include "merge_types.h"

namespace lsbm {
namespace {

constexpr uint64_t kMaxSequenceNumber = (1ull << 56) - 1;  // common/dbformat.h
constexpr uint32_t kTypeDeletion = 0, kTypeValue = 1;
constexpr uint32_t kCmpInternalKey = 1;  // LSBM_CMP_INTERNAL_KEY

// Compare of the comparator; under the internal-key one both lengths are >= 8
__device__ __forceinline__ int key_compare(uint32_t cmp, gcu8 a, uint64_t alen, gcu8 b, uint64_t blen) {
  if (cmp != kCmpInternalKey) return bytes_compare(a, alen, b, blen);
  const int c = bytes_compare(a, alen - 8, b, blen - 8);
  if (c) return c;
  return tag_compare(load8(a + (alen - 8)), load8(b + (blen - 8)));  // the tag descending (common/dbformat.cc)
}

// the run that owns entry e < n: the last r with run_first[r] <= e (run_first
// was checked: it starts at 0, ends at n and does not decrease)
__device__ __forceinline__ uint32_t run_of(const MergePlanArgs& a, uint64_t e) {
  uint32_t lo = 0, hi = a.n_runs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.run_first[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool key_ok(const MergePlanArgs& a, uint64_t ka, uint64_t kb) {
  return ka <= kb && kb <= a.e.keys_size && (a.cmp != kCmpInternalKey || kb - ka >= 8);
}

// exclusive sums of (c, b) over the workgroup's lanes in lane order, and the totals
__device__ __forceinline__ void block_excl_scan(uint64_t c, uint64_t b, uint64_t (*lds)[2], uint64_t& ec, uint64_t& eb,
                                                uint64_t& tc, uint64_t& tb) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t ic = wave_incl_scan(c, lane), ib = wave_incl_scan(b, lane);
  if (lane == 63) {
    lds[w][0] = ic;
    lds[w][1] = ib;
  }
  __syncthreads();
  uint64_t oc = 0, ob = 0;
  tc = 0;
  tb = 0;
  for (uint32_t i = 0; i < (uint32_t)kMergeWaves; i++) {
    if (i < w) {
      oc += lds[i][0];
      ob += lds[i][1];
    }
    tc += lds[i][0];
    tb += lds[i][1];
  }
  __syncthreads();  // (the row is free for the caller's next round)
  ec = oc + ic - c;
  eb = ob + ib - b;
}

// ---------------------------------------------------------------- plan

__global__ __launch_bounds__(64) void merge_init_kernel(MergePlanArgs a) {
  const uint32_t r = threadIdx.x;
  uint32_t st = kMergeOk;
  if (r < a.n_runs) {
    const uint64_t lo = a.run_first[r], hi = a.run_first[r + 1];
    if (lo > hi || hi > a.e.n || (r == 0 && lo != 0) || (r + 1 == a.n_runs && hi != a.e.n)) st = kMergeBadInput;
    a.run_status[r] = st;
  }
  const bool bad = __ballot(st != kMergeOk) != 0;
  if (r == 0) {
    *a.s.err = bad ? 1u : 0u;
    a.counts[0] = 0;
    a.counts[1] = 0;
  }
}

__global__ __launch_bounds__(kMergeThreads) void merge_check_kernel(MergePlanArgs a) {
  if (*a.s.err) return;  // the runs themselves are not defined
  const uint64_t e = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (e >= a.e.n) return;
  const uint32_t r = run_of(a, e);
  const uint64_t end = a.run_first[r + 1];
  const uint64_t ka = a.e.key_offsets[e], kb = a.e.key_offsets[e + 1];
  uint32_t st = kMergeOk;
  if (!key_ok(a, ka, kb)) {
    st = kMergeBadInput;
  } else if (e + 1 < end) {
    const uint64_t nb = a.e.key_offsets[e + 2];  // (e + 2 <= n: the successor is an entry of the run)
    if (key_ok(a, kb, nb) && key_compare(a.cmp, gptr(a.e.keys, ka), kb - ka, gptr(a.e.keys, kb), nb - kb) > 0)
      st = kMergeUnsorted;
  }
  if (st != kMergeOk) {
    atomicMax(&a.run_status[r], st);
    atomicOr(a.s.err, 1u);
  }
}

// key e's bound in [lo, hi) of another run: with ties the first entry above
// key e (an earlier run wins ties: its keys <= key e come first), without the
// first entry not below it
__device__ __forceinline__ uint64_t bound_in(const MergePlanArgs& a, uint64_t lo, uint64_t hi, gcu8 k, uint64_t klen,
                                             bool ties) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t ma = a.e.key_offsets[mid], mlen = a.e.key_offsets[mid + 1] - ma;
    const int c = key_compare(a.cmp, gptr(a.e.keys, ma), mlen, k, klen);
    if (c < 0 || (ties && c == 0)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the slot of run r's first sample: run starts are at least one slot apart
__device__ __forceinline__ uint64_t slot_base(const MergePlanArgs& a, uint32_t r) {
  return a.run_first[r] / kMergeSample + r;
}

__global__ __launch_bounds__(kMergeThreads) void merge_sample_kernel(MergePlanArgs a) {
  if (*a.s.err) return;
  const uint64_t t = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (t >= a.s.n_slots) return;
  // the run of slot t: the last r with slot_base(r) <= t (slot_base(0) = 0, strictly increasing)
  uint32_t r = 0, hi = a.n_runs;
  while (hi - r > 1) {
    const uint32_t mid = r + ((hi - r) >> 1);
    if (slot_base(a, mid) <= t) r = mid; else hi = mid;
  }
  const uint64_t first = a.run_first[r], e = first + (t - slot_base(a, r)) * kMergeSample;
  if (e >= a.run_first[r + 1]) return;  // a slot between two runs
  const uint64_t ka = a.e.key_offsets[e], klen = a.e.key_offsets[e + 1] - ka;
  const gcu8 k = gptr(a.e.keys, ka);
  for (uint32_t s = 0; s < a.n_runs; s++)
    if (s != r) a.s.bounds[t * a.n_runs + s] = bound_in(a, a.run_first[s], a.run_first[s + 1], k, klen, s < r);
}

__global__ __launch_bounds__(kMergeThreads) void merge_rank_kernel(MergePlanArgs a) {
  if (*a.s.err) return;
  const uint64_t e = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (e >= a.e.n) return;
  const uint32_t r = run_of(a, e);
  const uint64_t ka = a.e.key_offsets[e], klen = a.e.key_offsets[e + 1] - ka;
  const gcu8 k = gptr(a.e.keys, ka);
  const uint64_t at = e - a.run_first[r];
  // the samples around e: its bounds lie between theirs (the run is sorted)
  const uint64_t t = slot_base(a, r) + at / kMergeSample;
  const bool is_sample = at % kMergeSample == 0;
  const bool has_next = a.run_first[r] + (at / kMergeSample + 1) * kMergeSample < a.run_first[r + 1];
  uint64_t rank = at;
  for (uint32_t s = 0; s < a.n_runs; s++) {
    if (s == r) continue;
    const uint64_t first = a.run_first[s], end = a.run_first[s + 1];
    uint64_t lo = first, hi = end;
    if (t + 1 < a.s.n_slots) {  // (always: the slots were counted with one to spare)
      const uint64_t b0 = a.s.bounds[t * a.n_runs + s];
      const uint64_t b1 = has_next ? a.s.bounds[(t + 1) * a.n_runs + s] : end;
      if (first <= b0 && b0 <= b1 && b1 <= end) {  // (else the whole run: scratch is not trusted)
        lo = b0;
        hi = is_sample ? b0 : b1;
      }
    }
    rank += bound_in(a, lo, hi, k, klen, s < r) - first;
  }
  if (rank < a.e.n) a.s.order[rank] = e;
}

// entry at merged position p and its key; false if the scratch does not hold an entry there
__device__ __forceinline__ bool entry_at(const MergePlanArgs& a, uint64_t p, uint64_t& e, uint64_t& ka, uint64_t& klen) {
  e = a.s.order[p];
  if (e >= a.e.n) return false;
  ka = a.e.key_offsets[e];
  klen = a.e.key_offsets[e + 1] - ka;
  return true;
}

__global__ __launch_bounds__(kMergeThreads) void merge_flag_kernel(MergePlanArgs a) {
  __shared__ uint64_t lds[kMergeWaves][2];
  const uint64_t p = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  uint32_t keep = 0;
  uint64_t e, ka, klen = 0;
  if (!*a.s.err && p < a.e.n && entry_at(a, p, e, ka, klen)) {
    keep = 1;
    if (a.flags & kMergeDrop) {  // (internal keys: every length is >= 8)
      const gcu8 k = gptr(a.e.keys, ka);
      const uint64_t tag = load8(k + (klen - 8));
      const uint32_t type = (uint32_t)(tag & 0xff);
      if (type <= kTypeValue) {  // ParseInternalKey; an error key is never hidden
        uint64_t last_seq = kMaxSequenceNumber, pe, pa, plen;
        if (p > 0 && entry_at(a, p - 1, pe, pa, plen)) {
          const gcu8 pk = gptr(a.e.keys, pa);
          const uint64_t ptag = load8(pk + (plen - 8));
          if ((ptag & 0xff) <= kTypeValue && bytes_compare(pk, plen - 8, k, klen - 8) == 0) last_seq = ptag >> 8;
        }
        const bool drop = last_seq <= a.smallest_snapshot ||
                          (type == kTypeDeletion && (tag >> 8) <= a.smallest_snapshot && (a.flags & kMergeBottomLevel));
        keep = drop ? 0u : 1u;
      }
    }
  }
  if (p < a.e.n) a.s.keep[p] = keep;
  uint64_t ec, eb, tc, tb;
  block_excl_scan(keep, keep ? klen : 0, lds, ec, eb, tc, tb);
  if (threadIdx.x == 0) {
    a.s.tiles[2 * (uint64_t)blockIdx.x] = tc;
    a.s.tiles[2 * (uint64_t)blockIdx.x + 1] = tb;
  }
}

__global__ __launch_bounds__(kMergeThreads) void merge_scan_kernel(MergePlanArgs a) {
  __shared__ uint64_t lds[kMergeWaves][2];
  uint64_t carry_c = 0, carry_b = 0;
  for (uint64_t base = 0; base < a.n_tiles; base += kMergeThreads) {
    const uint64_t t = base + threadIdx.x;
    const uint64_t c = t < a.n_tiles ? a.s.tiles[2 * t] : 0, b = t < a.n_tiles ? a.s.tiles[2 * t + 1] : 0;
    uint64_t ec, eb, tc, tb;
    block_excl_scan(c, b, lds, ec, eb, tc, tb);
    if (t < a.n_tiles) {
      a.s.tiles[2 * t] = carry_c + ec;
      a.s.tiles[2 * t + 1] = carry_b + eb;
    }
    carry_c += tc;
    carry_b += tb;
  }
  if (threadIdx.x == 0) {
    if (*a.s.err || carry_c > a.e.n) carry_c = carry_b = 0;
    a.counts[0] = carry_c;
    a.counts[1] = carry_b;
    a.out_key_offsets[carry_c] = carry_b;  // the slot after the last output entry
  }
}

__global__ __launch_bounds__(kMergeThreads) void merge_emit_kernel(MergePlanArgs a) {
  __shared__ uint64_t lds[kMergeWaves][2];
  if (*a.s.err) return;  // (uniform)
  const uint64_t p = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  uint32_t keep = 0;
  uint64_t e = 0, ka, klen = 0;
  if (p < a.e.n && a.s.keep[p] && entry_at(a, p, e, ka, klen)) keep = 1;
  uint64_t ec, eb, tc, tb;
  block_excl_scan(keep, keep ? klen : 0, lds, ec, eb, tc, tb);
  const uint64_t j = a.s.tiles[2 * (uint64_t)blockIdx.x] + ec;
  if (keep && j < a.e.n) {
    a.source[j] = e;
    a.out_key_offsets[j] = a.s.tiles[2 * (uint64_t)blockIdx.x + 1] + eb;
  }
}

// ---------------------------------------------------------------- gather

__global__ __launch_bounds__(kMergeThreads) void merge_gather_kernel(MergeGatherArgs a) {
  __shared__ uint64_t s_out[kMergeWaves][65];  // the wave's entries' first output bytes, then the range's end
  __shared__ uint64_t s_src[kMergeWaves][64];  // and their keys' places in the input
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t n_out = a.counts[0], total = a.counts[1];
  if (n_out > a.entries_cap || total > a.out_keys_cap || n_out > a.e.n) {  // (uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(a.status, kMergeNoRoom);
    return;
  }
  const uint64_t j0 = ((uint64_t)blockIdx.x * kMergeWaves + w) * 64;
  if (j0 > n_out) return;  // (wave-uniform; the waves share no LDS row)
  const uint64_t j = j0 + lane;
  const uint32_t cnt = (uint32_t)(n_out - j0 < 64 ? n_out - j0 : 64);
  if (j == n_out) a.out_key_offsets[j] = total;
  uint64_t o = 0, o1 = 0, ka = 0;
  bool bad = false;
  if (lane < cnt) {
    o = a.plan_key_offsets[j];
    o1 = a.plan_key_offsets[j + 1];
    const uint64_t src = a.source[j];
    bad = o > o1 || o1 > total || src >= a.e.n;
    if (!bad) {
      ka = a.e.key_offsets[src];
      const uint64_t kb = a.e.key_offsets[src + 1];
      bad = ka > kb || kb > a.e.keys_size || kb - ka != o1 - o;
    }
    if (!bad) {
      a.out_key_offsets[j] = o;
      a.out_values[2 * j] = a.e.values[2 * src];
      a.out_values[2 * j + 1] = a.e.values[2 * src + 1];
    }
  }
  if (__ballot(bad) != 0) {  // not a plan of these entries: no key byte of the wave is moved
    if (lane == 0) atomicMax(a.status, kMergeBadInput);
    return;
  }
  if (cnt == 0) return;
  const uint64_t lo = __shfl(o, 0), hi = __shfl(o1, (int)cnt - 1);
  s_out[w][lane] = lane < cnt ? o : hi;
  if (lane == 0) s_out[w][64] = hi;
  s_src[w][lane] = ka;
  wave_phase();
  // chunk c is output bytes [8c, 8c + 8) cut to [lo, hi): every byte has one lane
  for (uint64_t c = (lo >> 3) + lane; (c << 3) < hi; c += 64) {
    const uint64_t q0 = (c << 3) > lo ? (c << 3) : lo;
    const uint64_t q1 = (c << 3) + 8 < hi ? (c << 3) + 8 : hi;
    // the entry of byte q0: the last l < cnt with s_out[l] <= q0 (s_out[0] = lo <= q0)
    uint32_t l = 0, h = cnt;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (s_out[w][mid] <= q0) l = mid; else h = mid;
    }
    if (q1 - q0 == 8 && q1 <= s_out[w][l + 1]) {
      const uint64_t x = load8(gptr(a.e.keys, s_src[w][l] + (q0 - s_out[w][l])));
      store8(gwptr(a.out_keys, q0), x);
    } else {
      for (uint64_t q = q0; q < q1; q++) {
        while (q >= s_out[w][l + 1]) l++;  // (q < hi = s_out[cnt]: stops at l < cnt)
        a.out_keys[q] = a.e.keys[s_src[w][l] + (q - s_out[w][l])];
      }
    }
  }
}

}  // namespace

hipError_t launch_merge_plan(const MergePlanArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(merge_init_kernel, dim3(1), dim3(64), 0, stream, a);
  if (a.e.n) {
    const dim3 grid((uint32_t)a.n_tiles), block(kMergeThreads);
    hipLaunchKernelGGL(merge_check_kernel, grid, block, 0, stream, a);
    const dim3 sample_grid((uint32_t)((a.s.n_slots + kMergeThreads - 1) / kMergeThreads));
    hipLaunchKernelGGL(merge_sample_kernel, sample_grid, block, 0, stream, a);
    hipLaunchKernelGGL(merge_rank_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(merge_flag_kernel, grid, block, 0, stream, a);
  }
  hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(kMergeThreads), 0, stream, a);
  if (a.e.n) hipLaunchKernelGGL(merge_emit_kernel, dim3((uint32_t)a.n_tiles), dim3(kMergeThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_merge_gather(const MergeGatherArgs& a, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  // one wave per 64 output entries, and the slot after the last one
  const uint64_t wgs = a.e.n / kMergeThreads + 1;
  hipLaunchKernelGGL(merge_gather_kernel, dim3((uint32_t)wgs), dim3(kMergeThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
