// table_pack_engine.cc -- the device entry points of include/lsbm_table_pack.h.
//
// Validates arguments, carves the scratch and launches table_pack_kernels.hip
// on the caller's stream.  Never packs on the CPU: without a usable device
// every entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_table_pack.h"
#include "engine_internal.h"
#include "table_pack_types.h"

namespace lsbm {

// launchers (table_pack_kernels.hip)
hipError_t launch_pack_plan(const PackPlanArgs& a, hipStream_t stream);
hipError_t launch_pack(const PackArgs& a, hipStream_t stream);

namespace {

uint64_t tiles_of(uint64_t n) { return (n + kPackThreads - 1) / kPackThreads; }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_block_pack_scratch_bytes(uint64_t n_blocks) {
  // the mover's pieces (u64) per block; a running sum per tile and the total
  return 8 * (n_blocks + tiles_of(n_blocks) + 1);
}

__attribute__((visibility("default"))) int lsbm_block_pack_plan_dev(
    const uint64_t* d_raw_len, const uint64_t* d_comp_len, uint64_t n_blocks, uint64_t first_offset, uint64_t gap,
    uint8_t* d_types, uint64_t* d_handles, uint64_t* d_end, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (n_blocks > LSBM_PACK_MAX_BLOCKS) return engine_fail(LSBM_ERR_INVALID, "too many blocks");
  if (!d_end || !d_scratch || (n_blocks && (!d_raw_len || !d_types || !d_handles)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (scratch_bytes < lsbm_block_pack_scratch_bytes(n_blocks) || (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_block_pack_scratch_bytes)");
  const Range outs[] = {{d_types, n_blocks}, {d_handles, 16 * n_blocks}, {d_end, 8}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_raw_len, 8 * n_blocks}, {d_comp_len, 8 * n_blocks}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  PackPlanArgs a = {};
  a.raw_len = d_raw_len;
  a.comp_len = d_comp_len;
  a.n = n_blocks;
  a.n_tiles = tiles_of(n_blocks);
  a.first_offset = first_offset;
  a.gap = gap;
  a.types = d_types;
  a.handles = d_handles;
  a.end = d_end;
  a.tiles = static_cast<uint64_t*>(d_scratch);
  const hipError_t e = launch_pack_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "pack plan kernels");
}

__attribute__((visibility("default"))) int lsbm_block_pack_dev(
    const uint8_t* d_raw, uint64_t raw_size, const uint64_t* d_raw_handles, const uint8_t* d_comp, uint64_t comp_size,
    const uint64_t* d_comp_offsets, const uint8_t* d_types, const uint64_t* d_handles, uint64_t n_blocks, uint64_t gap,
    uint8_t* d_out, uint64_t out_size, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (n_blocks > LSBM_PACK_MAX_BLOCKS) return engine_fail(LSBM_ERR_INVALID, "too many blocks");
  if ((!d_raw && raw_size) || (!d_comp && comp_size) || (!d_out && out_size) ||
      (n_blocks && (!d_types || !d_handles || !d_status || !d_scratch)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (n_blocks &&
      (scratch_bytes < lsbm_block_pack_scratch_bytes(n_blocks) || (reinterpret_cast<uint64_t>(d_scratch) & 7u)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_block_pack_scratch_bytes)");
  const Range outs[] = {{d_out, out_size}, {d_status, 4 * n_blocks}, {d_scratch, n_blocks ? scratch_bytes : 0}};
  const Range ins[] = {{d_raw, raw_size},       {d_raw_handles, 16 * n_blocks}, {d_comp, comp_size},
                       {d_comp_offsets, 8 * n_blocks}, {d_types, n_blocks},     {d_handles, 16 * n_blocks}};
  if (any_overlap(outs, ins) || overlap(d_out, out_size, d_status, 4 * n_blocks) ||
      overlap(d_out, out_size, d_scratch, n_blocks ? scratch_bytes : 0) ||
      overlap(d_status, 4 * n_blocks, d_scratch, n_blocks ? scratch_bytes : 0))
    return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  PackArgs a = {};
  a.raw = d_raw;
  a.raw_size = raw_size;
  a.raw_handles = d_raw_handles;
  a.comp = d_comp;
  a.comp_size = comp_size;
  a.comp_offsets = d_comp_offsets;
  a.types = d_types;
  a.handles = d_handles;
  a.n = n_blocks;
  a.n_tiles = tiles_of(n_blocks);
  a.gap = gap;
  a.out = d_out;
  a.out_size = out_size;
  a.status = d_status;
  a.pieces = static_cast<uint64_t*>(d_scratch);
  a.tiles = a.pieces + n_blocks;
  const hipError_t e = launch_pack(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "pack kernels");
}

}  // extern "C"
