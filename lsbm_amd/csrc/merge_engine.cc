// merge_engine.cc -- the device entry points of include/lsbm_merge.h.
//
// Validates arguments, carves plan's scratch and launches merge_kernels.hip on
// the caller's stream.  Never merges on the CPU: without a usable device every
// entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_merge.h"
#include "engine_internal.h"
#include "merge_types.h"

namespace lsbm {

// launchers (merge_kernels.hip)
hipError_t launch_merge_plan(const MergePlanArgs& a, hipStream_t stream);
hipError_t launch_merge_gather(const MergeGatherArgs& a, hipStream_t stream);

namespace {

uint64_t tiles_of(uint64_t n_entries) { return (n_entries + kMergeThreads - 1) / kMergeThreads; }
// sample slots: run r's start at run_first[r] / kMergeSample + r, so no two runs share one
uint64_t slots_of(uint64_t n_entries, uint64_t n_runs) { return n_entries / kMergeSample + n_runs + 1; }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_merge_scratch_bytes(uint64_t n_entries, uint64_t n_runs) {
  if (n_runs > LSBM_MERGE_MAX_RUNS) n_runs = LSBM_MERGE_MAX_RUNS;  // (more is refused by the plan)
  // order (u64) per entry; {entries, key bytes} per tile; keep (u32) per entry, rounded up; the error word;
  // a bound per sample slot and run
  return 8 * n_entries + 16 * tiles_of(n_entries) + 8 * ((n_entries + 1) / 2) + 8 +
         8 * n_runs * slots_of(n_entries, n_runs);
}

__attribute__((visibility("default"))) int lsbm_merge_plan_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries,
    const uint64_t* d_run_first, uint64_t n_runs, int cmp, uint32_t flags, uint64_t smallest_snapshot,
    uint64_t* d_source, uint64_t* d_out_key_offsets, uint64_t* d_counts, uint32_t* d_run_status, void* d_scratch,
    uint64_t scratch_bytes, void* stream) {
  if (cmp != LSBM_CMP_BYTEWISE && cmp != LSBM_CMP_INTERNAL_KEY) return engine_fail(LSBM_ERR_INVALID, "unknown comparator");
  if (flags & ~(LSBM_MERGE_DROP | LSBM_MERGE_BOTTOM_LEVEL)) return engine_fail(LSBM_ERR_INVALID, "unknown flag");
  if ((flags & LSBM_MERGE_DROP) && cmp != LSBM_CMP_INTERNAL_KEY)
    return engine_fail(LSBM_ERR_INVALID, "the drop rule needs internal keys (LSBM_CMP_INTERNAL_KEY)");
  if (n_runs > LSBM_MERGE_MAX_RUNS) return engine_fail(LSBM_ERR_INVALID, "more than LSBM_MERGE_MAX_RUNS runs");
  if (n_runs == 0 && n_entries) return engine_fail(LSBM_ERR_INVALID, "entries without a run");
  if (n_entries > LSBM_MERGE_MAX_ENTRIES) return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (!d_key_offsets || !d_run_first || !d_out_key_offsets || !d_counts || !d_scratch || (!d_keys && keys_size) ||
      (!d_source && n_entries) || (!d_run_status && n_runs))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (scratch_bytes < lsbm_merge_scratch_bytes(n_entries, n_runs) || (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_merge_scratch_bytes)");
  const Range outs[] = {{d_source, 8 * n_entries}, {d_out_key_offsets, 8 * (n_entries + 1)}, {d_counts, 16},
                        {d_run_status, 4 * n_runs}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_run_first, 8 * (n_runs + 1)}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MergePlanArgs a = {};
  a.e.keys = d_keys;
  a.e.keys_size = keys_size;
  a.e.key_offsets = d_key_offsets;
  a.e.n = n_entries;
  a.run_first = d_run_first;
  a.n_runs = (uint32_t)n_runs;
  a.cmp = (uint32_t)cmp;
  a.flags = flags;
  a.smallest_snapshot = smallest_snapshot;
  a.n_tiles = tiles_of(n_entries);
  a.source = d_source;
  a.out_key_offsets = d_out_key_offsets;
  a.counts = d_counts;
  a.run_status = d_run_status;
  uint64_t* s = static_cast<uint64_t*>(d_scratch);
  a.s.order = s;
  a.s.tiles = s + n_entries;
  a.s.keep = reinterpret_cast<uint32_t*>(s + n_entries + 2 * a.n_tiles);
  a.s.err = reinterpret_cast<uint32_t*>(s + n_entries + 2 * a.n_tiles + (n_entries + 1) / 2);
  a.s.bounds = s + n_entries + 2 * a.n_tiles + (n_entries + 1) / 2 + 1;
  a.s.n_slots = slots_of(n_entries, n_runs);
  const hipError_t e = launch_merge_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "merge plan kernels");
}

__attribute__((visibility("default"))) int lsbm_merge_gather_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, const uint64_t* d_values,
    uint64_t n_entries, const uint64_t* d_source, const uint64_t* d_plan_key_offsets, const uint64_t* d_counts,
    uint8_t* d_out_keys, uint64_t out_keys_cap, uint64_t* d_out_key_offsets, uint64_t* d_out_values,
    uint64_t entries_cap, uint32_t* d_status, void* stream) {
  if (n_entries > LSBM_MERGE_MAX_ENTRIES || entries_cap > LSBM_MERGE_MAX_ENTRIES)
    return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (!d_key_offsets || !d_plan_key_offsets || !d_counts || !d_out_key_offsets || !d_status || (!d_keys && keys_size) ||
      (!d_values && n_entries) || (!d_source && n_entries) || (!d_out_keys && out_keys_cap) ||
      (!d_out_values && entries_cap))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_out_keys, out_keys_cap}, {d_out_key_offsets, 8 * (entries_cap + 1)},
                        {d_out_values, 16 * entries_cap}, {d_status, 4}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_values, 16 * n_entries},
                       {d_source, 8 * n_entries}, {d_plan_key_offsets, 8 * (n_entries + 1)}, {d_counts, 16}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MergeGatherArgs a = {};
  a.e.keys = d_keys;
  a.e.keys_size = keys_size;
  a.e.key_offsets = d_key_offsets;
  a.e.values = d_values;
  a.e.n = n_entries;
  a.source = d_source;
  a.plan_key_offsets = d_plan_key_offsets;
  a.counts = d_counts;
  a.out_keys = d_out_keys;
  a.out_keys_cap = out_keys_cap;
  a.out_key_offsets = d_out_key_offsets;
  a.out_values = d_out_values;
  a.entries_cap = entries_cap;
  a.status = d_status;
  const hipError_t e = launch_merge_gather(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "merge_gather_kernel");
}

}  // extern "C"
