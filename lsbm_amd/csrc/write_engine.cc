// write_engine.cc -- the device entry points of include/lsbm_write.h.
//
// Validates arguments, carves the scratch, zeroes the call's status word and
// launches write_kernels.hip on the caller's stream.  Never encodes, groups or
// frames on the CPU: without a usable device every entry point returns
// LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_write.h"
#include "engine_internal.h"
#include "write_types.h"

namespace lsbm {

// launchers (write_kernels.hip)
hipError_t launch_write_sizes(const WrSizesArgs& a, int writer_grid, hipStream_t stream);
hipError_t launch_write_group(const WrGroupArgs& a, int writer_grid, hipStream_t stream);
hipError_t launch_write_build(const WrBuildArgs& a, int check_grid, int group_grid, int move_grid, hipStream_t stream);
hipError_t launch_frame_plan(const WrFrameArgs& a, int record_grid, hipStream_t stream);
hipError_t launch_frame(const WrFrameArgs& a, int record_grid, int move_grid, hipStream_t stream);

namespace {

constexpr uint64_t kMaxCount = 1ull << 31;  // ops, writers: below this
constexpr uint64_t kMaxBytes = 1ull << 62;  // sizes, caps, log offsets: below this
constexpr uint64_t kMaxRecords = 1ull << 36;
constexpr uint64_t kWgsPerCu = 8;

uint64_t tiles_of(uint64_t n) { return (n + kWrThreads - 1) / kWrThreads; }
uint64_t pad8(uint64_t bytes) { return (bytes + 7) & ~7ull; }
uint64_t sizes_scratch(uint64_t n_ops) { return 8 * (tiles_of(n_ops) + 1); }
uint64_t group_scratch(uint64_t n_writers) { return 3 * pad8(4 * n_writers) + 8; }

bool scratch_ok(const void* p, uint64_t have, uint64_t need) {
  return p && have >= need && !(reinterpret_cast<uint64_t>(p) & 7u);
}

int finish(hipError_t e, const char* what) { return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, what); }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_write_scratch_bytes(uint64_t n_ops, uint64_t n_writers) {
  return std::max(sizes_scratch(n_ops), group_scratch(n_writers));
}

__attribute__((visibility("default"))) int lsbm_write_sizes_dev(
    const uint8_t* d_types, const uint64_t* d_key_offsets, uint64_t keys_size, const uint64_t* d_values,
    uint64_t value_image_size, uint64_t n_ops, const uint64_t* d_batch_first, uint64_t n_writers, uint64_t* d_op_sum,
    uint64_t* d_batch_sum, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (n_ops >= kMaxCount || n_writers >= kMaxCount) return engine_fail(LSBM_ERR_INVALID, "too many ops or writers");
  if (keys_size >= kMaxBytes || value_image_size >= kMaxBytes) return engine_fail(LSBM_ERR_INVALID, "image too large");
  if (!d_key_offsets || !d_batch_first || !d_op_sum || !d_batch_sum || !d_status || (n_ops && (!d_types || !d_values)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, sizes_scratch(n_ops)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_write_scratch_bytes)");
  const Range outs[] = {{d_op_sum, 8 * (n_ops + 1)}, {d_batch_sum, 8 * (n_writers + 1)}, {d_status, 4},
                        {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_types, n_ops}, {d_key_offsets, 8 * (n_ops + 1)}, {d_values, 16 * n_ops},
                       {d_batch_first, 8 * (n_writers + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WrSizesArgs a = {};
  a.o.types = d_types;
  a.o.keys_size = keys_size;
  a.o.key_offsets = d_key_offsets;
  a.o.value_image_size = value_image_size;
  a.o.values = d_values;
  a.o.n = n_ops;
  a.o.batch_first = d_batch_first;
  a.o.n_writers = n_writers;
  a.op_sum = d_op_sum;
  a.batch_sum = d_batch_sum;
  a.status = d_status;
  a.tiles = static_cast<uint64_t*>(d_scratch);
  a.n_tiles = tiles_of(n_ops);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_write_sizes(a, grid_for(cus, n_writers + 1, kWrThreads, kWgsPerCu), s);
  return finish(e, "write sizes kernels");
}

__attribute__((visibility("default"))) int lsbm_write_group_dev(
    const uint64_t* d_batch_sum, uint64_t n_writers, const uint8_t* d_sync, uint64_t* d_group_first,
    uint8_t* d_group_sync, uint64_t groups_cap, uint64_t* d_n_groups, uint32_t* d_status, void* d_scratch,
    uint64_t scratch_bytes, void* stream) {
  if (n_writers >= kMaxCount || groups_cap >= kMaxCount) return engine_fail(LSBM_ERR_INVALID, "too many writers");
  if (!d_batch_sum || !d_group_first || !d_n_groups || !d_status || (groups_cap && !d_group_sync))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, group_scratch(n_writers)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_write_scratch_bytes)");
  const Range outs[] = {{d_group_first, 8 * (groups_cap + 1)}, {d_group_sync, groups_cap}, {d_n_groups, 8},
                        {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_batch_sum, 8 * (n_writers + 1)}, {d_sync, n_writers}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WrGroupArgs a = {};
  a.batch_sum = d_batch_sum;
  a.n = n_writers;
  a.sync = d_sync;
  a.group_first = d_group_first;
  a.group_sync = d_group_sync;
  a.groups_cap = groups_cap;
  a.n_groups = d_n_groups;
  a.status = d_status;
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  const uint64_t row = pad8(4 * n_writers);
  a.link = reinterpret_cast<uint32_t*>(p);
  a.nsync = reinterpret_cast<uint32_t*>(p + row);
  a.starts = reinterpret_cast<uint32_t*>(p + 2 * row);
  a.count = reinterpret_cast<uint64_t*>(p + 3 * row);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_write_group(a, grid_for(cus, n_writers, kWrThreads, kWgsPerCu), s);
  return finish(e, "write group kernels");
}

__attribute__((visibility("default"))) int lsbm_write_build_dev(
    const uint8_t* d_types, const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
    const uint8_t* d_value_image, uint64_t value_image_size, const uint64_t* d_values, uint64_t n_ops,
    const uint64_t* d_batch_first, uint64_t n_writers, const uint64_t* d_op_sum, const uint64_t* d_group_first,
    uint64_t n_groups, uint64_t last_sequence, uint8_t* d_reps, uint64_t reps_cap, uint64_t* d_records,
    uint64_t* d_seq_counts, uint64_t* d_last_sequence, uint32_t* d_status, void* stream) {
  if (n_ops >= kMaxCount || n_writers >= kMaxCount || n_groups >= kMaxCount)
    return engine_fail(LSBM_ERR_INVALID, "too many ops, writers or groups");
  if (keys_size >= kMaxBytes || value_image_size >= kMaxBytes || reps_cap >= kMaxBytes)
    return engine_fail(LSBM_ERR_INVALID, "image too large");
  if (!d_key_offsets || !d_batch_first || !d_op_sum || !d_group_first || !d_last_sequence || !d_status ||
      (n_ops && (!d_types || !d_values)) || (!d_keys && keys_size) || (!d_value_image && value_image_size) ||
      (!d_reps && reps_cap) || (n_groups && (!d_records || !d_seq_counts)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_reps, reps_cap}, {d_records, 16 * n_groups}, {d_seq_counts, 16 * n_groups},
                        {d_last_sequence, 8}, {d_status, 4}};
  const Range ins[] = {{d_types, n_ops}, {d_keys, keys_size}, {d_key_offsets, 8 * (n_ops + 1)},
                       {d_value_image, value_image_size}, {d_values, 16 * n_ops},
                       {d_batch_first, 8 * (n_writers + 1)}, {d_op_sum, 8 * (n_ops + 1)},
                       {d_group_first, 8 * (n_groups + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WrBuildArgs a = {};
  a.o.types = d_types;
  a.o.keys = d_keys;
  a.o.keys_size = keys_size;
  a.o.key_offsets = d_key_offsets;
  a.o.value_image = d_value_image;
  a.o.value_image_size = value_image_size;
  a.o.values = d_values;
  a.o.n = n_ops;
  a.o.batch_first = d_batch_first;
  a.o.n_writers = n_writers;
  a.op_sum = d_op_sum;
  a.group_first = d_group_first;
  a.n_groups = n_groups;
  a.last_sequence = last_sequence;
  a.reps = d_reps;
  a.reps_cap = reps_cap;
  a.records = d_records;
  a.seq_counts = d_seq_counts;
  a.new_last_sequence = d_last_sequence;
  a.status = d_status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_write_build(a, grid_for(cus, std::max(n_ops, n_writers), kWrThreads, kWgsPerCu),
                           grid_for(cus, n_groups, kWrThreads, kWgsPerCu),
                           grid_for(cus, reps_cap / kWrChunk + 2, kWrThreads, kWgsPerCu), s);
  return finish(e, "write build kernels");
}

__attribute__((visibility("default"))) int lsbm_log_frame_plan_dev(uint64_t image_size, const uint64_t* d_records,
                                                                   uint64_t n_records, uint64_t log_offset,
                                                                   uint64_t* d_frag_first, uint64_t* d_rec_start,
                                                                   uint32_t* d_status, void* stream) {
  if (n_records > kMaxRecords) return engine_fail(LSBM_ERR_INVALID, "too many records");
  if (image_size >= kMaxBytes || log_offset >= kMaxBytes) return engine_fail(LSBM_ERR_INVALID, "image or offset too large");
  if (!d_frag_first || !d_rec_start || !d_status || (n_records && !d_records))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_frag_first, 8 * (n_records + 1)}, {d_rec_start, 8 * (n_records + 1)}, {d_status, 4}};
  const Range ins[] = {{d_records, 16 * n_records}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WrFrameArgs a = {};
  a.image_size = image_size;
  a.records = d_records;
  a.n = n_records;
  a.log_offset = log_offset;
  a.frag_first = d_frag_first;
  a.rec_start = d_rec_start;
  a.status = d_status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_frame_plan(a, grid_for(cus, n_records, kWrThreads, kWgsPerCu), s);
  return finish(e, "log frame plan kernels");
}

__attribute__((visibility("default"))) int lsbm_log_frame_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n_records, uint64_t log_offset,
    const uint64_t* d_frag_first, const uint64_t* d_rec_start, uint8_t* d_out, uint64_t out_cap, uint64_t* d_headers,
    uint64_t headers_cap, uint32_t* d_status, void* stream) {
  if (n_records > kMaxRecords) return engine_fail(LSBM_ERR_INVALID, "too many records");
  if (image_size >= kMaxBytes || log_offset >= kMaxBytes || out_cap >= kMaxBytes || headers_cap >= kMaxBytes / 8)
    return engine_fail(LSBM_ERR_INVALID, "image, offset or cap too large");
  if (!d_frag_first || !d_rec_start || !d_status || (n_records && !d_records) || (!d_image && image_size) ||
      (!d_out && out_cap) || (!d_headers && headers_cap))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_out, out_cap}, {d_headers, 8 * headers_cap}, {d_status, 4}};
  const Range ins[] = {{d_image, image_size}, {d_records, 16 * n_records}, {d_frag_first, 8 * (n_records + 1)},
                       {d_rec_start, 8 * (n_records + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WrFrameArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.records = d_records;
  a.n = n_records;
  a.log_offset = log_offset;
  a.frag_first = const_cast<uint64_t*>(d_frag_first);
  a.rec_start = const_cast<uint64_t*>(d_rec_start);
  a.out = d_out;
  a.out_cap = out_cap;
  a.headers = d_headers;
  a.headers_cap = headers_cap;
  a.status = d_status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_frame(a, grid_for(cus, n_records, kWrThreads, kWgsPerCu),
                     grid_for(cus, std::max(out_cap / kWrChunk + 2, n_records), kWrThreads, kWgsPerCu), s);
  return finish(e, "log frame kernels");
}

}  // extern "C"
