// probe_kernels.hip -- gfx950 kernels of the probe plan of LSbM's buffered Get
// (include/lsbm_probe.h): the walk of Version::Get (lsbm/version_set.cc:349-623)
// over a level's sorted tables under covered_by_del, covered_by_ins,
// covered_by_head and checkwb, as a per-query list of slots.
//
// probe_check_kernel        one lane per slot, cursor offset and lookup key:
//                           the slot table is sorted by (level, kind) with one
//                           DEL, HEAD and INS a level at most; the offsets do
//                           not decrease and stay inside their buffers.
// probe_cand_check_kernel   one lane per candidate byte: a known code.
// probe_count_kernel        one lane per query: the number of its probes.
// probe_first_check_kernel  one lane per query: d_probe_first steps by the
//                           counts and ends inside probe_cap.
// probe_emit_kernel         one lane per query: its probes' slots, in order.
//
// The candidates are slot-major (cand[s * n + q]): the lanes of a wave are 64
// consecutive queries, so each step of a lane's pass over its slots reads 64
// consecutive bytes, one cache line a wave.  The slot table, the use lengths
// and the cursor offsets are the same for every lane (scalar loads).  A level's
// slots are read twice by the emit kernel (what the gates say, then the slots
// they let through); the second pass hits the cache.
//
// Every kernel that reads a key or a candidate runs after the check kernels of
// its call on the same stream and leaves at once when they set the status
// word, so bytes are addressed only through offsets that were checked, and the
// emit kernel stores only inside [probe_first[q], probe_first[q + 1]), which
// the first-check kernel has placed inside probe_cap.  Every loop advances.
// No LDS, no spin-waits, no cross-workgroup state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"       // gcu8, gptr, global_index
#include "key_compare_device.h"  // bytes_compare
#include "probe_types.h"

namespace lsbm {
namespace {

__device__ __forceinline__ bool is_probe(uint32_t c) { return c == kCandMay || c == kCandErr; }

__global__ __launch_bounds__(kProbeThreads) void probe_check_kernel(ProbeArgs a) {
  const uint64_t i = global_index<kProbeThreads>();
  bool bad = false;
  if (i < a.n_slots) {
    const uint32_t info = a.slot_info[i], level = info >> 8, kind = info & 0xff;
    bad = level >= kProbeLevels || kind > kSlotIns || ((level == 0) != (kind == kSlotLevel0));
    if (i > 0) {
      const uint32_t prev = a.slot_info[i - 1];
      const bool one = kind == kSlotDel || kind == kSlotHead || kind == kSlotIns;
      // (kind | level << 8 is the sort key itself)
      bad = bad || info < prev || (info == prev && one);
    }
  }
  if (i < kProbeLevels) {
    const uint64_t lo = a.cursor_offsets[i], hi = a.cursor_offsets[i + 1];
    bad = bad || lo > hi || hi > a.cursor_size;
  }
  if (i < a.n) {
    const uint64_t lo = a.key_offsets[i], hi = a.key_offsets[i + 1];
    bad = bad || lo > hi || hi > a.keys_size || hi - lo < 8;
  }
  if (bad) atomicMax(a.status, kProbeBadInput);
}

__global__ __launch_bounds__(kProbeThreads) void probe_cand_check_kernel(ProbeArgs a) {
  const uint64_t i = global_index<kProbeThreads>();
  if (i >= a.n_slots * a.n) return;
  if (gptr(a.cand, i)[0] > kCandErr) atomicMax(a.status, kProbeBadInput);
}

// The probes of query q; with kEmit their slots go to probe_slot[at...].
template <bool kEmit>
__device__ __forceinline__ uint32_t probe_walk(const ProbeArgs& a, uint64_t q, uint64_t at) {
  const uint64_t n = a.n, n_slots = a.n_slots;
  const gcu8 cand = gptr(a.cand, q);
  uint32_t count = 0;
  uint64_t s = 0;
  // Level 0: every file that overlaps, then the insertion table's file (:364-379)
  for (; s < n_slots && (a.slot_info[s] >> 8) == 0; s++) {
    if (is_probe(cand[s * n])) {
      if (kEmit) a.probe_slot[at + count] = (uint32_t)s;
      count++;
    }
  }
  const uint64_t ka = a.key_offsets[q], ulen = a.key_offsets[q + 1] - ka - 8;
  const gcu8 u = gptr(a.keys, ka);
  while (s < n_slots) {
    const uint32_t level = a.slot_info[s] >> 8;
    // what the gates say, and how many tables of the two walks would be read
    uint32_t c_del = kCandNone, c_head = kCandNone, c_ins = kCandNone, n_wb = 0, n_rest = 0;
    uint64_t e = s;
    for (; e < n_slots; e++) {
      const uint32_t info = a.slot_info[e];
      if ((info >> 8) != level) break;
      const uint32_t kind = info & 0xff, c = cand[e * n];
      if (kind == kSlotDel) {
        c_del = c;
      } else if (kind == kSlotHead) {
        c_head = c;
      } else if (kind == kSlotIns) {
        c_ins = c;
      } else if (kind == kSlotWb) {
        n_wb += is_probe(c);
      } else {
        n_rest += is_probe(c);
      }
    }
    const uint32_t use = a.use_len[level];
    bool checkwb = false;
    if (a.wb_enabled[level]) {
      const uint64_t co = a.cursor_offsets[level], cl = a.cursor_offsets[level + 1] - co;
      checkwb = bytes_compare(u, ulen, gptr(a.cursor_keys, co), cl) > 0;
    }
    const bool covered_by_del = use == 0 && c_del != kCandNone;
    const bool del_step = covered_by_del && c_del == kCandMay;
    const bool ins_step = c_ins == kCandMay;
    const bool head_ok = ins_step && !covered_by_del && use > 0 && c_head == kCandMay;
    const bool wb = checkwb && (del_step || (ins_step && !covered_by_del && (use == 0 || head_ok)));
    if (kEmit) {
      for (uint64_t t = s; t < e; t++) {
        const uint32_t kind = a.slot_info[t] & 0xff;
        bool take;
        if (kind == kSlotDel) {
          take = del_step;
        } else if (kind == kSlotHead) {
          take = head_ok;
        } else if (kind == kSlotIns) {
          take = ins_step;
        } else if (kind == kSlotWb) {
          take = wb && is_probe(cand[t * n]);
        } else {
          take = ins_step && is_probe(cand[t * n]);
        }
        if (take) {
          a.probe_slot[at + count] = (uint32_t)t;
          count++;
        }
      }
    } else {
      count += (wb ? n_wb : 0) + del_step + head_ok + (ins_step ? n_rest + 1 : 0);
    }
    s = e;
  }
  return count;
}

__global__ __launch_bounds__(kProbeThreads) void probe_count_kernel(ProbeArgs a) {
  const uint64_t q = global_index<kProbeThreads>();
  if (q >= a.n || *a.status) return;
  a.count[q] = probe_walk<false>(a, q, 0);
}

__global__ __launch_bounds__(kProbeThreads) void probe_first_check_kernel(ProbeArgs a) {
  const uint64_t q = global_index<kProbeThreads>();
  if (q > a.n || *a.status) return;
  if (q == a.n) {
    if (a.probe_first[q] > a.probe_cap) atomicMax(a.status, kProbeNoRoom);
    return;
  }
  const uint64_t lo = a.probe_first[q], hi = a.probe_first[q + 1];
  if (lo > hi || hi - lo != probe_walk<false>(a, q, 0)) atomicMax(a.status, kProbeBadInput);
}

__global__ __launch_bounds__(kProbeThreads) void probe_emit_kernel(ProbeArgs a) {
  const uint64_t q = global_index<kProbeThreads>();
  if (q >= a.n || *a.status) return;
  probe_walk<true>(a, q, a.probe_first[q]);
}

uint32_t groups(uint64_t n) { return (uint32_t)((n + kProbeThreads - 1) / kProbeThreads); }

hipError_t launch_checks(const ProbeArgs& a, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  uint64_t items = a.n_slots > a.n ? a.n_slots : a.n;
  if (items < kProbeLevels) items = kProbeLevels;
  hipLaunchKernelGGL(probe_check_kernel, dim3(groups(items)), dim3(kProbeThreads), 0, stream, a);
  if (a.n_slots * a.n)
    hipLaunchKernelGGL(probe_cand_check_kernel, dim3(groups(a.n_slots * a.n)), dim3(kProbeThreads), 0, stream, a);
  return hipSuccess;
}

}  // namespace

hipError_t launch_probe_plan(const ProbeArgs& a, hipStream_t stream) {
  const hipError_t e = launch_checks(a, stream);
  if (e != hipSuccess) return e;
  if (a.n) hipLaunchKernelGGL(probe_count_kernel, dim3(groups(a.n)), dim3(kProbeThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_probe_emit(const ProbeArgs& a, hipStream_t stream) {
  const hipError_t e = launch_checks(a, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(probe_first_check_kernel, dim3(groups(a.n + 1)), dim3(kProbeThreads), 0, stream, a);
  if (a.n) hipLaunchKernelGGL(probe_emit_kernel, dim3(groups(a.n)), dim3(kProbeThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
