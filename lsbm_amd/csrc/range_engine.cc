// range_engine.cc -- the device entry points of include/lsbm_range.h.
//
// Validates arguments and launches range_kernels.hip on the caller's stream.
// Never plans or counts anything on the CPU: without a usable device every
// entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_range.h"
#include "engine_internal.h"
#include "range_types.h"

namespace lsbm {

// launchers (range_kernels.hip)
hipError_t launch_range_plan(const RangePlanArgs& a, hipStream_t stream);
hipError_t launch_range_emit(const RangePlanArgs& a, hipStream_t stream);
hipError_t launch_range_count(const RangeCountArgs& a, hipStream_t stream);

namespace {

constexpr uint64_t kMaxQueries = 1ull << 31;  // per call
constexpr uint64_t kMaxSlots = 1ull << 20;
constexpr uint64_t kMaxRuns = 1ull << 31;     // run entries are stored as 32-bit words
constexpr uint64_t kMaxPairs = 1ull << 33;    // the count kernel's grid: four pairs a workgroup
constexpr uint64_t kMaxEntries = 1ull << 31;  // a count is a 32-bit word

static_assert(kRangeLevels == LSBM_RANGE_LEVELS && kRangeCursors == LSBM_RANGE_CURSORS,
              "range_types.h and lsbm_range.h disagree");
static_assert(kRsIns == LSBM_RANGE_SLOT_INS && kRangeSole == LSBM_RANGE_SOLE && kRangeLast == LSBM_RANGE_LAST,
              "range_types.h and lsbm_range.h disagree");

int range_keys(const uint8_t* d_start_keys, uint64_t start_keys_size, const uint64_t* d_start_offsets,
               const uint8_t* d_end_keys, uint64_t end_keys_size, const uint64_t* d_end_offsets, uint64_t n_queries,
               RangeKeys* k) {
  if (n_queries > kMaxQueries) return engine_fail(LSBM_ERR_INVALID, "too many queries");
  if ((!d_start_keys && start_keys_size) || (!d_end_keys && end_keys_size) ||
      (n_queries && (!d_start_offsets || !d_end_offsets)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  *k = {d_start_keys, start_keys_size, d_start_offsets, d_end_keys, end_keys_size, d_end_offsets, n_queries};
  return LSBM_OK;
}

// the checks both plan calls share; fills every input field of `a`
int plan_args(const uint32_t* d_slot_info, uint64_t n_slots, const uint64_t* d_run_first, uint64_t n_runs,
              const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets,
              const uint32_t* d_use_len, const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys,
              uint64_t cursor_keys_size, const uint64_t* d_cursor_offsets, uint32_t* d_status, RangePlanArgs* a) {
  if (n_slots > kMaxSlots || n_runs > kMaxRuns) return engine_fail(LSBM_ERR_INVALID, "too many slots or files");
  if (!d_status || !d_use_len || !d_wb_enabled || !d_cursor_offsets || !d_run_first || !d_bound_offsets ||
      (!d_cursor_keys && cursor_keys_size) || (!d_bounds && bounds_size) || (n_slots && !d_slot_info))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  a->slot_info = d_slot_info;
  a->n_slots = n_slots;
  a->run_first = d_run_first;
  a->n_runs = n_runs;
  a->bounds = d_bounds;
  a->bounds_size = bounds_size;
  a->bound_offsets = d_bound_offsets;
  a->use_len = d_use_len;
  a->wb_enabled = d_wb_enabled;
  a->cursor_keys = d_cursor_keys;
  a->cursor_size = cursor_keys_size;
  a->cursor_offsets = d_cursor_offsets;
  a->status = d_status;
  return LSBM_OK;
}

}  // namespace
}  // namespace lsbm

using namespace lsbm;

// the input ranges both plan calls share, by their parameter names
#define RANGE_PLAN_INPUTS                                                                                       \
  Range{d_slot_info, 4 * n_slots}, Range{d_run_first, 8 * (n_slots + 1)}, Range{d_bounds, bounds_size},         \
      Range{d_bound_offsets, 8 * (2 * n_runs + 1)}, Range{d_use_len, 4 * kRangeLevels},                         \
      Range{d_wb_enabled, 4 * kRangeLevels}, Range{d_cursor_keys, cursor_keys_size},                            \
      Range{d_cursor_offsets, 8 * (kRangeCursors + 1)}, Range{d_start_keys, start_keys_size},                   \
      Range{d_start_offsets, 8 * (n_queries + 1)}, Range{d_end_keys, end_keys_size},                            \
      Range{d_end_offsets, 8 * (n_queries + 1)}

extern "C" {

__attribute__((visibility("default"))) int lsbm_range_plan_dev(
    const uint32_t* d_slot_info, uint64_t n_slots, const uint64_t* d_run_first, uint64_t n_runs,
    const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets, const uint32_t* d_use_len,
    const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys, uint64_t cursor_keys_size,
    const uint64_t* d_cursor_offsets, const uint8_t* d_start_keys, uint64_t start_keys_size,
    const uint64_t* d_start_offsets, const uint8_t* d_end_keys, uint64_t end_keys_size, const uint64_t* d_end_offsets,
    uint64_t n_queries, uint32_t* d_count, uint32_t* d_status, void* stream) {
  RangePlanArgs a = {};
  int rc = range_keys(d_start_keys, start_keys_size, d_start_offsets, d_end_keys, end_keys_size, d_end_offsets,
                      n_queries, &a.q);
  if (rc != LSBM_OK) return rc;
  rc = plan_args(d_slot_info, n_slots, d_run_first, n_runs, d_bounds, bounds_size, d_bound_offsets, d_use_len,
                 d_wb_enabled, d_cursor_keys, cursor_keys_size, d_cursor_offsets, d_status, &a);
  if (rc != LSBM_OK) return rc;
  if (n_queries && !d_count) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_count, 4 * n_queries}, {d_status, 4}};
  const Range ins[] = {RANGE_PLAN_INPUTS};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  a.count = d_count;
  const hipError_t e = launch_range_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "range_plan_kernel");
}

__attribute__((visibility("default"))) int lsbm_range_emit_dev(
    const uint32_t* d_slot_info, uint64_t n_slots, const uint64_t* d_run_first, uint64_t n_runs,
    const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets, const uint32_t* d_use_len,
    const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys, uint64_t cursor_keys_size,
    const uint64_t* d_cursor_offsets, const uint8_t* d_start_keys, uint64_t start_keys_size,
    const uint64_t* d_start_offsets, const uint8_t* d_end_keys, uint64_t end_keys_size, const uint64_t* d_end_offsets,
    uint64_t n_queries, const uint64_t* d_pair_first, uint32_t* d_pair_run, uint32_t* d_pair_flags, uint64_t pair_cap,
    uint32_t* d_checked, uint32_t* d_status, void* stream) {
  RangePlanArgs a = {};
  int rc = range_keys(d_start_keys, start_keys_size, d_start_offsets, d_end_keys, end_keys_size, d_end_offsets,
                      n_queries, &a.q);
  if (rc != LSBM_OK) return rc;
  rc = plan_args(d_slot_info, n_slots, d_run_first, n_runs, d_bounds, bounds_size, d_bound_offsets, d_use_len,
                 d_wb_enabled, d_cursor_keys, cursor_keys_size, d_cursor_offsets, d_status, &a);
  if (rc != LSBM_OK) return rc;
  if (pair_cap > kMaxPairs) return engine_fail(LSBM_ERR_INVALID, "too many pairs");
  if (!d_pair_first || (pair_cap && (!d_pair_run || !d_pair_flags)) || (n_queries && !d_checked))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_pair_run, 4 * pair_cap}, {d_pair_flags, 4 * pair_cap}, {d_checked, 4 * n_queries},
                        {d_status, 4}};
  const Range ins[] = {RANGE_PLAN_INPUTS, {d_pair_first, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  a.pair_first = d_pair_first;
  a.pair_run = d_pair_run;
  a.pair_flags = d_pair_flags;
  a.pair_cap = pair_cap;
  a.checked = d_checked;
  const hipError_t e = launch_range_emit(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "range_emit_kernel");
}

__attribute__((visibility("default"))) int lsbm_range_count_dev(
    const uint8_t* d_index_keys, uint64_t index_keys_size, const uint64_t* d_index_offsets, uint64_t n_entries,
    const uint64_t* d_file_first_entry, const uint32_t* d_file_state, uint64_t n_files, const uint8_t* d_start_keys,
    uint64_t start_keys_size, const uint64_t* d_start_offsets, const uint8_t* d_end_keys, uint64_t end_keys_size,
    const uint64_t* d_end_offsets, uint64_t n_queries, const uint64_t* d_pair_first, const uint32_t* d_pair_file,
    const uint32_t* d_pair_flags, uint64_t n_pairs, uint32_t* d_pair_count, uint32_t* d_pair_error,
    uint32_t* d_found, uint64_t* d_total, uint32_t* d_status, void* stream) {
  RangeCountArgs a = {};
  int rc = range_keys(d_start_keys, start_keys_size, d_start_offsets, d_end_keys, end_keys_size, d_end_offsets,
                      n_queries, &a.q);
  if (rc != LSBM_OK) return rc;
  if (n_pairs > kMaxPairs || n_entries > kMaxEntries || n_files > kMaxRuns)
    return engine_fail(LSBM_ERR_INVALID, "too many pairs, entries or files");
  if (!d_status || !d_pair_first || !d_file_first_entry || !d_index_offsets || (!d_index_keys && index_keys_size) ||
      (n_files && !d_file_state) || (n_pairs && (!d_pair_file || !d_pair_flags || !d_pair_count || !d_pair_error)) ||
      (n_queries && (!d_found || !d_total)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_pair_count, 4 * n_pairs}, {d_pair_error, 4 * n_pairs}, {d_found, 4 * n_queries},
                        {d_total, 8 * n_queries}, {d_status, 4}};
  const Range ins[] = {{d_index_keys, index_keys_size}, {d_index_offsets, 8 * (n_entries + 1)},
                       {d_file_first_entry, 8 * (n_files + 1)}, {d_file_state, 4 * n_files},
                       {d_start_keys, start_keys_size}, {d_start_offsets, 8 * (n_queries + 1)},
                       {d_end_keys, end_keys_size}, {d_end_offsets, 8 * (n_queries + 1)},
                       {d_pair_first, 8 * (n_queries + 1)}, {d_pair_file, 4 * n_pairs}, {d_pair_flags, 4 * n_pairs}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  a.index_keys = d_index_keys;
  a.index_size = index_keys_size;
  a.index_offsets = d_index_offsets;
  a.n_entries = n_entries;
  a.file_first = d_file_first_entry;
  a.file_state = d_file_state;
  a.n_files = n_files;
  a.pair_first = d_pair_first;
  a.pair_file = d_pair_file;
  a.pair_flags = d_pair_flags;
  a.n_pairs = n_pairs;
  a.pair_count = d_pair_count;
  a.pair_error = d_pair_error;
  a.found = d_found;
  a.total = d_total;
  a.status = d_status;
  const hipError_t e = launch_range_count(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "range_count_kernel");
}

}  // extern "C"
