// block_build_engine.cc -- the device entry points of include/lsbm_block_build.h.
//
// Validates arguments, carves plan's scratch, sizes the grids and launches
// block_build_kernels.hip on the caller's stream.  Never builds a block on the
// CPU: without a usable device every entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_block_build.h"
#include "block_build_types.h"
#include "engine_internal.h"

namespace lsbm {

// launchers (block_build_kernels.hip)
hipError_t launch_block_plan(const PlanArgs& a, int entry_grid, int table_wave_grid, int table_grid, hipStream_t stream);
hipError_t launch_block_build(const BuildArgs& a, int grid, hipStream_t stream);
hipError_t launch_index_build(const IndexArgs& a, int grid, hipStream_t stream);

}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_block_plan_scratch_bytes(uint64_t n_entries, uint64_t n_tables) {
  // sizes (2 x u32), link, bytes, starts per entry; counts and last per table
  return 32 * n_entries + 16 * n_tables + 16;
}

__attribute__((visibility("default"))) int lsbm_block_plan_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, const uint64_t* d_values,
    uint64_t n_entries, const uint64_t* d_table_first, uint64_t n_tables, uint64_t block_size,
    uint32_t restart_interval, uint64_t* d_block_first, uint64_t* d_block_bytes, uint64_t blocks_cap,
    uint64_t* d_table_block_first, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (!d_key_offsets || !d_table_first || !d_block_first || !d_table_block_first || !d_scratch ||
      (!d_keys && keys_size) || (!d_values && n_entries) || (!d_block_bytes && blocks_cap) || (!d_status && n_tables))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (restart_interval == 0) return engine_fail(LSBM_ERR_INVALID, "restart_interval must be at least 1");
  if (block_size == 0) return engine_fail(LSBM_ERR_INVALID, "block_size must be at least 1");
  if (n_entries > (1ull << 56) || n_tables > (1ull << 56)) return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (scratch_bytes < lsbm_block_plan_scratch_bytes(n_entries, n_tables) || (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_block_plan_scratch_bytes)");
  const Range outs[] = {{d_block_first, 8 * (blocks_cap + 1)}, {d_block_bytes, 8 * blocks_cap},
                        {d_table_block_first, 8 * (n_tables + 1)}, {d_status, 4 * n_tables}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_values, 16 * n_entries},
                       {d_table_first, 8 * (n_tables + 1)}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  PlanArgs a = {};
  a.e.keys = d_keys;
  a.e.keys_size = keys_size;
  a.e.key_offsets = d_key_offsets;
  a.e.values = d_values;
  a.e.n = n_entries;
  a.table_first = d_table_first;
  a.n_tables = n_tables;
  a.block_size = block_size;
  a.restart_interval = restart_interval;
  a.block_first = d_block_first;
  a.block_bytes = d_block_bytes;
  a.blocks_cap = blocks_cap;
  a.table_block_first = d_table_block_first;
  a.status = d_status;
  uint64_t* s = static_cast<uint64_t*>(d_scratch);
  a.s.sizes = reinterpret_cast<uint32_t*>(s);
  a.s.link = s + n_entries;
  a.s.bytes = s + 2 * n_entries;
  a.s.starts = s + 3 * n_entries;
  a.s.counts = s + 4 * n_entries;
  a.s.last = s + 4 * n_entries + n_tables;
  const hipError_t e = launch_block_plan(a, grid_for(cus, n_entries, kBuildThreads, 8), grid_for(cus, n_tables, kBuildWaves, 4),
                                         grid_for(cus, n_tables, 1, 8), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "block_plan kernels");
}

__attribute__((visibility("default"))) int lsbm_block_build_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, const uint64_t* d_values,
    const uint8_t* d_value_image, uint64_t value_image_size, uint64_t n_entries, const uint64_t* d_block_first,
    uint64_t n_blocks, uint32_t restart_interval, uint8_t* d_out, uint64_t out_size, const uint64_t* d_out_handles,
    uint64_t* d_built_bytes, uint32_t* d_status, void* stream) {
  if (restart_interval == 0) return engine_fail(LSBM_ERR_INVALID, "restart_interval must be at least 1");
  if (n_blocks == 0) return LSBM_OK;
  if (!d_key_offsets || !d_block_first || !d_out_handles || !d_status || (!d_keys && keys_size) ||
      (!d_values && n_entries) || (!d_value_image && value_image_size) || (!d_out && out_size))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (n_entries > (1ull << 56) || n_blocks > (1ull << 56)) return engine_fail(LSBM_ERR_INVALID, "too many entries");
  const Range outs[] = {{d_out, out_size}, {d_built_bytes, 8 * n_blocks}, {d_status, 4 * n_blocks}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_values, 16 * n_entries},
                       {d_value_image, value_image_size}, {d_block_first, 8 * (n_blocks + 1)},
                       {d_out_handles, 16 * n_blocks}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  BuildArgs a = {};
  a.e.keys = d_keys;
  a.e.keys_size = keys_size;
  a.e.key_offsets = d_key_offsets;
  a.e.values = d_values;
  a.e.value_image = d_value_image;
  a.e.value_image_size = value_image_size;
  a.e.n = n_entries;
  a.block_first = d_block_first;
  a.n_blocks = n_blocks;
  a.restart_interval = restart_interval;
  a.out = d_out;
  a.out_size = out_size;
  a.out_handles = d_out_handles;
  a.built_bytes = d_built_bytes;
  a.status = d_status;
  // 4 workgroups per CU: the build kernels' LDS tiles, 4 x 32 KiB of a CU's 160 KiB
  const hipError_t e = launch_block_build(a, grid_for(cus, n_blocks, kBuildWaves, 4), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "block_build_kernel");
}

__attribute__((visibility("default"))) int lsbm_index_block_build_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries,
    const uint64_t* d_block_first, uint64_t n_blocks, const uint64_t* d_table_block_first, uint64_t n_tables,
    const uint64_t* d_data_handles, int cmp, uint8_t* d_out, uint64_t out_size, const uint64_t* d_out_handles,
    uint64_t* d_built_bytes, uint32_t* d_status, void* stream) {
  if (cmp != LSBM_CMP_BYTEWISE && cmp != LSBM_CMP_INTERNAL_KEY) return engine_fail(LSBM_ERR_INVALID, "unknown comparator");
  if (n_tables == 0) return LSBM_OK;
  if (!d_key_offsets || !d_block_first || !d_table_block_first || !d_built_bytes || !d_status ||
      (!d_keys && keys_size) || (!d_data_handles && n_blocks) || (d_out && !d_out_handles))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (n_entries > (1ull << 56) || n_blocks > (1ull << 56) || n_tables > (1ull << 56))
    return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (!d_out) out_size = 0;
  const Range outs[] = {{d_out, out_size}, {d_built_bytes, 8 * n_tables}, {d_status, 4 * n_tables}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_block_first, 8 * (n_blocks + 1)},
                       {d_table_block_first, 8 * (n_tables + 1)}, {d_data_handles, 16 * n_blocks},
                       {d_out_handles, d_out ? 16 * n_tables : 0}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  IndexArgs a = {};
  a.e.keys = d_keys;
  a.e.keys_size = keys_size;
  a.e.key_offsets = d_key_offsets;
  a.e.n = n_entries;
  a.block_first = d_block_first;
  a.n_blocks = n_blocks;
  a.table_block_first = d_table_block_first;
  a.n_tables = n_tables;
  a.data_handles = d_data_handles;
  a.cmp = (uint32_t)cmp;
  a.out = d_out;
  a.out_size = out_size;
  a.out_handles = d_out_handles;
  a.built_bytes = d_built_bytes;
  a.status = d_status;
  const hipError_t e = launch_index_build(a, grid_for(cus, n_tables, kBuildWaves, 4), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "index_build_kernel");
}

}  // extern "C"
