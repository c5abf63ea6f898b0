// iter_engine.cc -- the device entry points of include/lsbm_iter.h.
//
// Validates arguments, carves plan's scratch and launches iter_kernels.hip on
// the caller's stream.  Never scans on the CPU: without a usable device every
// entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_iter.h"
#include "engine_internal.h"
#include "iter_types.h"

namespace lsbm {

// launchers (iter_kernels.hip)
hipError_t launch_dbiter_plan(const IterPlanArgs& a, hipStream_t stream);
hipError_t launch_dbiter_range(const IterRangeArgs& a, hipStream_t stream);
hipError_t launch_dbiter_emit(const IterEmitArgs& a, hipStream_t stream);

namespace {

uint64_t tiles_of(uint64_t n_entries) { return (n_entries + kIterThreads - 1) / kIterThreads; }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_dbiter_scratch_bytes(uint64_t n_entries) {
  // kIterTileWords words per tile; a flag byte per entry, rounded up to a word
  return 8 * kIterTileWords * tiles_of(n_entries) + 8 * ((n_entries + 7) / 8) + 8;
}

__attribute__((visibility("default"))) int lsbm_dbiter_plan_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries, uint64_t snapshot,
    uint64_t* d_source, uint64_t* d_out_key_offsets, uint64_t* d_counts, uint64_t* d_yield_rank,
    uint64_t* d_corrupt_rank, uint64_t* d_first, int64_t* d_back, uint32_t* d_status, void* d_scratch,
    uint64_t scratch_bytes, void* stream) {
  if (n_entries > LSBM_DBITER_MAX_ENTRIES) return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (snapshot >= (1ull << 56)) return engine_fail(LSBM_ERR_INVALID, "snapshot is a 56-bit sequence number");
  if (!d_key_offsets || !d_out_key_offsets || !d_counts || !d_yield_rank || !d_corrupt_rank || !d_status ||
      !d_scratch || (!d_keys && keys_size) || (n_entries && (!d_source || !d_first || !d_back)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (scratch_bytes < lsbm_dbiter_scratch_bytes(n_entries) || (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_dbiter_scratch_bytes)");
  const Range outs[] = {{d_source, 8 * n_entries},           {d_out_key_offsets, 8 * (n_entries + 1)},
                        {d_counts, 24},                      {d_yield_rank, 8 * (n_entries + 1)},
                        {d_corrupt_rank, 8 * (n_entries + 1)}, {d_first, 8 * n_entries},
                        {d_back, 8 * n_entries},             {d_status, 4},
                        {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  IterPlanArgs a = {};
  a.e = {d_keys, keys_size, d_key_offsets, n_entries};
  a.snapshot = snapshot;
  a.n_tiles = tiles_of(n_entries);
  a.source = d_source;
  a.out_key_offsets = d_out_key_offsets;
  a.counts = d_counts;
  a.yield_rank = d_yield_rank;
  a.corrupt_rank = d_corrupt_rank;
  a.first = d_first;
  a.back = d_back;
  a.status = d_status;
  a.tiles = static_cast<uint64_t*>(d_scratch);
  a.flags = reinterpret_cast<uint8_t*>(a.tiles + kIterTileWords * a.n_tiles);
  const hipError_t e = launch_dbiter_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "dbiter plan kernels");
}

__attribute__((visibility("default"))) int lsbm_dbiter_range_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries, uint64_t snapshot,
    const uint64_t* d_live, const uint64_t* d_live_key_offsets, const uint64_t* d_counts, const uint64_t* d_yield_rank,
    const uint64_t* d_corrupt_rank, const uint64_t* d_first, const int64_t* d_back, const uint64_t* d_value_prefix,
    const uint8_t* d_lo_keys, uint64_t lo_keys_size, const uint64_t* d_lo_offsets, const uint8_t* d_lo_present,
    const uint8_t* d_hi_keys, uint64_t hi_keys_size, const uint64_t* d_hi_offsets, const uint8_t* d_hi_present,
    uint64_t n_queries, uint64_t limit, const uint64_t* d_limits, int reverse, uint64_t* d_j_begin, uint64_t* d_count,
    uint32_t* d_scan_status, uint64_t* d_key_bytes, uint64_t* d_value_bytes, uint32_t* d_status, void* stream) {
  if (n_entries > LSBM_DBITER_MAX_ENTRIES || n_queries > LSBM_DBITER_MAX_QUERIES)
    return engine_fail(LSBM_ERR_INVALID, "too many entries or queries");
  if (snapshot >= (1ull << 56)) return engine_fail(LSBM_ERR_INVALID, "snapshot is a 56-bit sequence number");
  if (!d_key_offsets || !d_live_key_offsets || !d_counts || !d_yield_rank || !d_corrupt_rank || !d_value_prefix ||
      !d_status || (!d_keys && keys_size) || (n_entries && (!d_live || !d_first || !d_back)) ||
      (!d_lo_keys && lo_keys_size) || (!d_hi_keys && hi_keys_size) ||
      (n_queries && (!d_lo_offsets || !d_j_begin || !d_count || !d_scan_status || !d_key_bytes || !d_value_bytes)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_j_begin, 8 * n_queries},   {d_count, 8 * n_queries},       {d_scan_status, 4 * n_queries},
                        {d_key_bytes, 8 * n_queries}, {d_value_bytes, 8 * n_queries}, {d_status, 4}};
  const Range ins[] = {{d_keys, keys_size},
                       {d_key_offsets, 8 * (n_entries + 1)},
                       {d_live, 8 * n_entries},
                       {d_live_key_offsets, 8 * (n_entries + 1)},
                       {d_counts, 24},
                       {d_yield_rank, 8 * (n_entries + 1)},
                       {d_corrupt_rank, 8 * (n_entries + 1)},
                       {d_first, 8 * n_entries},
                       {d_back, 8 * n_entries},
                       {d_value_prefix, 8},
                       {d_lo_keys, lo_keys_size},
                       {d_lo_offsets, 8 * (n_queries + 1)},
                       {d_lo_present, n_queries},
                       {d_hi_keys, hi_keys_size},
                       {d_hi_offsets, 8 * (n_queries + 1)},
                       {d_hi_present, n_queries},
                       {d_limits, 8 * n_queries}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  IterRangeArgs a = {};
  a.e = {d_keys, keys_size, d_key_offsets, n_entries};
  a.snapshot = snapshot;
  a.v = {d_live, d_live_key_offsets, d_counts, d_yield_rank, d_corrupt_rank, d_first, d_back, d_value_prefix};
  a.lo_keys = d_lo_keys;
  a.lo_size = lo_keys_size;
  a.lo_offsets = d_lo_offsets;
  a.lo_present = d_lo_present;
  a.hi_keys = d_hi_keys;
  a.hi_size = hi_keys_size;
  a.hi_offsets = d_hi_offsets;
  a.hi_present = d_hi_present;
  a.n_queries = n_queries;
  a.limit = limit;
  a.limits = d_limits;
  a.reverse = reverse ? 1u : 0u;
  a.j_begin = d_j_begin;
  a.count = d_count;
  a.scan_status = d_scan_status;
  a.key_bytes = d_key_bytes;
  a.value_bytes = d_value_bytes;
  a.status = d_status;
  const hipError_t e = launch_dbiter_range(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "iter_range_kernel");
}

__attribute__((visibility("default"))) int lsbm_dbiter_emit_dev(
    const uint64_t* d_j_begin, const uint64_t* d_entry_first, const uint64_t* d_key_first,
    const uint64_t* d_value_first, uint64_t n_queries, int reverse, const uint8_t* d_live_keys,
    uint64_t live_keys_size, const uint64_t* d_live_key_offsets, const uint64_t* d_live_values, uint64_t n_live,
    const uint64_t* d_value_prefix, const uint8_t* d_image, uint64_t image_size, uint8_t* d_out_keys,
    uint64_t out_keys_cap, uint64_t* d_out_key_offsets, uint8_t* d_out_values, uint64_t out_values_cap,
    uint64_t* d_out_value_offsets, uint64_t entries_cap, uint32_t* d_status, void* stream) {
  if (n_live > LSBM_DBITER_MAX_ENTRIES || entries_cap > LSBM_DBITER_MAX_ENTRIES ||
      n_queries > LSBM_DBITER_MAX_QUERIES)
    return engine_fail(LSBM_ERR_INVALID, "too many entries or queries");
  if (!d_entry_first || !d_key_first || !d_value_first || !d_live_key_offsets || !d_value_prefix ||
      !d_out_key_offsets || !d_out_value_offsets || !d_status || (n_queries && !d_j_begin) ||
      (!d_live_keys && live_keys_size) || (n_live && !d_live_values) || (!d_image && image_size) ||
      (!d_out_keys && out_keys_cap) || (!d_out_values && out_values_cap))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_out_keys, out_keys_cap},
                        {d_out_key_offsets, 8 * (entries_cap + 1)},
                        {d_out_values, out_values_cap},
                        {d_out_value_offsets, 8 * (entries_cap + 1)},
                        {d_status, 4}};
  const Range ins[] = {{d_j_begin, 8 * n_queries},
                       {d_entry_first, 8 * (n_queries + 1)},
                       {d_key_first, 8 * (n_queries + 1)},
                       {d_value_first, 8 * (n_queries + 1)},
                       {d_live_keys, live_keys_size},
                       {d_live_key_offsets, 8 * (n_live + 1)},
                       {d_live_values, 16 * n_live},
                       {d_value_prefix, 8 * (n_live + 1)},
                       {d_image, image_size}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  IterEmitArgs a = {};
  a.j_begin = d_j_begin;
  a.entry_first = d_entry_first;
  a.key_first = d_key_first;
  a.value_first = d_value_first;
  a.n_queries = n_queries;
  a.reverse = reverse ? 1u : 0u;
  a.live_keys = d_live_keys;
  a.live_keys_size = live_keys_size;
  a.live_key_offsets = d_live_key_offsets;
  a.live_values = d_live_values;
  a.n_live = n_live;
  a.value_prefix = d_value_prefix;
  a.image = d_image;
  a.image_size = image_size;
  a.out_keys = d_out_keys;
  a.out_keys_cap = out_keys_cap;
  a.out_key_offsets = d_out_key_offsets;
  a.out_values = d_out_values;
  a.out_values_cap = out_values_cap;
  a.out_value_offsets = d_out_value_offsets;
  a.entries_cap = entries_cap;
  a.status = d_status;
  const hipError_t e = launch_dbiter_emit(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "iter_emit_out_kernel");
}

}  // extern "C"
