// get_engine.cc -- the device entry points of include/lsbm_get.h.
//
// Validates arguments and launches get_kernels.hip on the caller's stream.
// Never looks anything up on the CPU: without a usable device every entry
// point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_get.h"
#include "engine_internal.h"
#include "get_types.h"

namespace lsbm {

// launchers (get_kernels.hip)
hipError_t launch_lookup_keys(const LookupArgs& a, hipStream_t stream);
hipError_t launch_memtable_get(const MemGetArgs& a, hipStream_t stream);
hipError_t launch_find_file(const FindFileArgs& a, hipStream_t stream);
hipError_t launch_save_value(const SaveArgs& a, hipStream_t stream);
hipError_t launch_slices_gather(const GatherArgs& a, hipStream_t stream);

namespace {

constexpr uint64_t kMaxQueries = 1ull << 31;  // per call
constexpr uint64_t kMaxEntries = 1ull << 36;  // memtable entries, files, (query, run) pairs

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) int lsbm_lookup_keys_dev(const uint8_t* d_user_keys, uint64_t user_keys_size,
                                                                const uint64_t* d_user_offsets, uint64_t n_queries,
                                                                uint64_t snapshot, const uint64_t* d_snapshots,
                                                                uint8_t* d_keys, uint64_t keys_cap,
                                                                uint64_t* d_key_offsets, uint32_t* d_status,
                                                                void* stream) {
  if (n_queries > kMaxQueries) return engine_fail(LSBM_ERR_INVALID, "too many queries");
  if (!d_user_offsets || !d_key_offsets || !d_status || (!d_user_keys && user_keys_size) || (!d_keys && keys_cap))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_keys, keys_cap}, {d_key_offsets, 8 * (n_queries + 1)}, {d_status, 4}};
  const Range ins[] = {{d_user_keys, user_keys_size}, {d_user_offsets, 8 * (n_queries + 1)},
                       {d_snapshots, 8 * n_queries}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  LookupArgs a = {};
  a.user_keys = d_user_keys;
  a.user_size = user_keys_size;
  a.user_offsets = d_user_offsets;
  a.n = n_queries;
  a.snapshot = snapshot;
  a.snapshots = d_snapshots;
  a.keys = d_keys;
  a.keys_cap = keys_cap;
  a.key_offsets = d_key_offsets;
  a.status = d_status;
  const hipError_t e = launch_lookup_keys(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "lookup_keys_kernel");
}

__attribute__((visibility("default"))) int lsbm_memtable_get_dev(
    const uint8_t* d_mem_keys, uint64_t mem_keys_size, const uint64_t* d_mem_key_offsets, const uint64_t* d_mem_values,
    uint64_t n_entries, const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_queries,
    int32_t source_id, uint32_t* d_verdict, uint64_t* d_value, int32_t* d_where, uint32_t* d_status, void* stream) {
  if (n_queries > kMaxQueries || n_entries > kMaxEntries) return engine_fail(LSBM_ERR_INVALID, "too many queries");
  if (!d_status || (!d_mem_keys && mem_keys_size) || (!d_keys && keys_size) ||
      (n_entries && (!d_mem_key_offsets || !d_mem_values)) ||
      (n_queries && (!d_key_offsets || !d_verdict || !d_value || !d_where)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_verdict, 4 * n_queries}, {d_value, 16 * n_queries}, {d_where, 4 * n_queries},
                        {d_status, 4}};
  const Range ins[] = {{d_mem_keys, mem_keys_size}, {d_mem_key_offsets, 8 * (n_entries + 1)},
                       {d_mem_values, 16 * n_entries}, {d_keys, keys_size}, {d_key_offsets, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  MemGetArgs a = {};
  a.q = {d_keys, keys_size, d_key_offsets, n_queries, source_id, d_verdict, d_value, d_where, d_status};
  a.mem_keys = d_mem_keys;
  a.mem_keys_size = mem_keys_size;
  a.mem_key_offsets = d_mem_key_offsets;
  a.mem_values = d_mem_values;
  a.n_entries = n_entries;
  const hipError_t e = launch_memtable_get(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "mem_get_kernel");
}

__attribute__((visibility("default"))) int lsbm_find_file_dev(
    const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets, uint64_t n_files,
    const uint64_t* d_run_first, const uint32_t* d_run_flags, const uint8_t* d_visible, uint64_t n_runs,
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_queries, int32_t* d_file,
    uint32_t* d_status, void* stream) {
  if (n_queries > kMaxQueries || n_files >= (1ull << 31) || n_runs > kMaxEntries ||
      (n_runs && n_queries > kMaxEntries / n_runs))
    return engine_fail(LSBM_ERR_INVALID, "too many queries, files or runs");
  if (!d_status || (!d_bounds && bounds_size) || (!d_keys && keys_size) || (n_files && (!d_bound_offsets || !d_visible)) ||
      (n_runs && (!d_run_first || !d_run_flags)) || (n_queries && !d_key_offsets) || (n_queries * n_runs && !d_file))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_file, 4 * n_queries * n_runs}, {d_status, 4}};
  const Range ins[] = {{d_bounds, bounds_size}, {d_bound_offsets, 8 * (2 * n_files + 1)},
                       {d_run_first, 8 * (n_runs + 1)}, {d_run_flags, 4 * n_runs}, {d_visible, n_files},
                       {d_keys, keys_size}, {d_key_offsets, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  FindFileArgs a = {};
  a.bounds = d_bounds;
  a.bounds_size = bounds_size;
  a.bound_offsets = d_bound_offsets;
  a.n_files = n_files;
  a.run_first = d_run_first;
  a.run_flags = d_run_flags;
  a.visible = d_visible;
  a.n_runs = n_runs;
  a.keys = d_keys;
  a.keys_size = keys_size;
  a.key_offsets = d_key_offsets;
  a.n = n_queries;
  a.file = d_file;
  a.status = d_status;
  const hipError_t e = launch_find_file(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "find_file_kernel");
}

__attribute__((visibility("default"))) int lsbm_save_value_dev(
    const uint32_t* d_state, const uint64_t* d_key_len, const uint8_t* d_found, uint64_t found_size,
    const uint64_t* d_found_offsets, const uint64_t* d_value_in, const uint8_t* d_keys, uint64_t keys_size,
    const uint64_t* d_key_offsets, uint64_t n_queries, int32_t source_id, uint32_t* d_verdict, uint64_t* d_value,
    int32_t* d_where, uint32_t* d_status, void* stream) {
  if (n_queries > kMaxQueries) return engine_fail(LSBM_ERR_INVALID, "too many queries");
  if (!d_status || (!d_found && found_size) || (!d_keys && keys_size) ||
      (n_queries && (!d_state || !d_key_len || !d_found_offsets || !d_value_in || !d_key_offsets || !d_verdict ||
                     !d_value || !d_where)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_verdict, 4 * n_queries}, {d_value, 16 * n_queries}, {d_where, 4 * n_queries},
                        {d_status, 4}};
  const Range ins[] = {{d_state, 4 * n_queries}, {d_key_len, 8 * n_queries}, {d_found, found_size},
                       {d_found_offsets, 8 * (n_queries + 1)}, {d_value_in, 16 * n_queries}, {d_keys, keys_size},
                       {d_key_offsets, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  SaveArgs a = {};
  a.q = {d_keys, keys_size, d_key_offsets, n_queries, source_id, d_verdict, d_value, d_where, d_status};
  a.state = d_state;
  a.key_len = d_key_len;
  a.found = d_found;
  a.found_size = found_size;
  a.found_offsets = d_found_offsets;
  a.value_in = d_value_in;
  const hipError_t e = launch_save_value(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "save_value_kernel");
}

__attribute__((visibility("default"))) int lsbm_slices_gather_dev(const uint8_t* d_image, uint64_t image_size,
                                                                  const uint64_t* d_slices, const int32_t* d_where,
                                                                  int32_t where_lo, int32_t where_hi, uint8_t* d_out,
                                                                  uint64_t out_cap, const uint64_t* d_out_offsets,
                                                                  uint64_t n_queries, uint32_t* d_status,
                                                                  void* stream) {
  if (n_queries > kMaxQueries) return engine_fail(LSBM_ERR_INVALID, "too many queries");
  if (!d_status || (!d_image && image_size) || (!d_out && out_cap) ||
      (n_queries && (!d_slices || !d_where || !d_out_offsets)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_out, out_cap}, {d_status, 4}};
  const Range ins[] = {{d_image, image_size}, {d_slices, 16 * n_queries}, {d_where, 4 * n_queries},
                       {d_out_offsets, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  GatherArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.slices = d_slices;
  a.where = d_where;
  a.where_lo = where_lo;
  a.where_hi = where_hi;
  a.out = d_out;
  a.out_cap = out_cap;
  a.out_offsets = d_out_offsets;
  a.n = n_queries;
  a.status = d_status;
  const hipError_t e = launch_slices_gather(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "slices_gather_kernel");
}

}  // extern "C"
