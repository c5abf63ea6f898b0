// block_engine.cc -- the device entry points of include/lsbm_block.h.
//
// Validates arguments, sizes the grid and launches block_kernels.hip on the
// caller's stream.  Never walks a block on the CPU: without a usable device
// every entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_block.h"
#include "block_types.h"
#include "engine_internal.h"

namespace lsbm {

// launchers (block_kernels.hip)
hipError_t launch_block_walk(const BlockWalkArgs& a, bool decode, int grid, hipStream_t stream);
hipError_t launch_block_seek(const BlockSeekArgs& a, int grid, hipStream_t stream);

namespace {

int walk(BlockWalkArgs& a, bool decode, void* stream) {
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  // 4 workgroups per CU: the walk kernels' LDS tiles, 4 x 32 KiB of a CU's 160 KiB
  // (decode's key caches: 48 KiB of LDS per workgroup, 3 per CU)
  const hipError_t e =
      launch_block_walk(a, decode, grid_for(cus, a.n, kBlockWaves, decode ? 3 : 4), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, decode ? "block_decode_kernel" : "block_scan_kernel");
}

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) int lsbm_block_scan_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles, uint64_t n_blocks,
    uint64_t* d_counts, uint32_t* d_status, void* stream) {
  if (n_blocks == 0) return LSBM_OK;
  if (!d_image || !d_handles || !d_counts || !d_status) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  BlockWalkArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.handles = d_handles;
  a.n = n_blocks;
  a.counts = d_counts;
  a.status = d_status;
  return walk(a, false, stream);
}

__attribute__((visibility("default"))) int lsbm_block_decode_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles, uint64_t n_blocks,
    const uint64_t* d_entry_base, const uint64_t* d_key_base, uint8_t* d_keys, uint64_t keys_cap,
    uint64_t* d_key_offsets, uint64_t* d_values, uint64_t entries_cap, uint64_t* d_counts,
    uint32_t* d_status, void* stream) {
  if (n_blocks == 0) return LSBM_OK;
  if (!d_image || !d_handles || !d_entry_base || !d_key_base || !d_key_offsets || !d_status ||
      (!d_keys && keys_cap) || (!d_values && entries_cap))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  BlockWalkArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.handles = d_handles;
  a.n = n_blocks;
  a.counts = d_counts;
  a.status = d_status;
  a.entry_base = d_entry_base;
  a.key_base = d_key_base;
  a.keys = d_keys;
  a.keys_cap = keys_cap;
  a.key_offsets = d_key_offsets;
  a.values = d_values;
  a.entries_cap = entries_cap;
  return walk(a, true, stream);
}

__attribute__((visibility("default"))) int lsbm_block_seek_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles, const void* d_keys,
    const uint64_t* d_key_offsets, uint64_t n_queries, int cmp, uint32_t flags, uint32_t* d_state,
    uint64_t* d_pos, uint64_t* d_key_len, uint64_t* d_value, uint64_t* d_handle_out, uint8_t* d_found,
    const uint64_t* d_found_offsets, uint64_t found_cap, void* stream) {
  if (n_queries == 0) return LSBM_OK;
  if (!d_image || !d_handles || !d_keys || !d_key_offsets || !d_state || !d_pos || !d_key_len || !d_value)
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (cmp != LSBM_CMP_BYTEWISE && cmp != LSBM_CMP_INTERNAL_KEY) return engine_fail(LSBM_ERR_INVALID, "unknown comparator");
  if (flags & ~LSBM_SEEK_VALUE_IS_HANDLE) return engine_fail(LSBM_ERR_INVALID, "unknown flags");
  if ((flags & LSBM_SEEK_VALUE_IS_HANDLE) && !d_handle_out)
    return engine_fail(LSBM_ERR_INVALID, "LSBM_SEEK_VALUE_IS_HANDLE needs d_handle_out");
  if (d_found && !d_found_offsets) return engine_fail(LSBM_ERR_INVALID, "d_found needs d_found_offsets");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  BlockSeekArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.handles = d_handles;
  a.keys = static_cast<const uint8_t*>(d_keys);
  a.key_offsets = d_key_offsets;
  a.n = n_queries;
  a.cmp = (uint32_t)cmp;
  a.flags = flags;
  a.state = d_state;
  a.pos = d_pos;
  a.key_len = d_key_len;
  a.value = d_value;
  a.handle_out = d_handle_out;
  a.found = d_found;
  a.found_offsets = d_found_offsets;
  a.found_cap = found_cap;
  const hipError_t e = launch_block_seek(a, grid_for(cus, n_queries, kBlockThreads, 8), static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "block_seek_kernel");
}

}  // extern "C"
