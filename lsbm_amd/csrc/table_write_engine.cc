// table_write_engine.cc -- the device entry points of include/lsbm_table_write.h.
//
// Validates arguments, carves the scratch and launches table_write_kernels.hip
// on the caller's stream.  Never lays out or sorts on the CPU: without a usable
// device every entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_table_write.h"
#include "engine_internal.h"
#include "table_write_types.h"

namespace lsbm {

// launchers (table_write_kernels.hip)
hipError_t launch_table_pack_plan(const TwPlanArgs& a, hipStream_t stream);
hipError_t launch_filter_layout(const TwFilterArgs& a, hipStream_t stream);
hipError_t launch_metaindex(const TwMetaArgs& a, hipStream_t stream);
hipError_t launch_table_place(const TwPlaceArgs& a, hipStream_t stream);
hipError_t launch_sort_segments(const SegSortArgs& a, hipStream_t stream);

namespace {

uint64_t tiles_of(uint64_t n) { return (n + kTwThreads - 1) / kTwThreads; }
uint64_t pad8(uint64_t bytes) { return (bytes + 7) & ~7ull; }

bool counts_ok(uint64_t n_blocks, uint64_t n_tables) {
  return n_blocks <= LSBM_TABLE_WRITE_MAX_BLOCKS && n_tables <= LSBM_TABLE_WRITE_MAX_TABLES;
}

bool scratch_ok(const void* d_scratch, uint64_t scratch_bytes, uint64_t n_blocks, uint64_t n_tables) {
  return d_scratch && scratch_bytes >= lsbm_table_write_scratch_bytes(n_blocks, n_tables) &&
         !(reinterpret_cast<uint64_t>(d_scratch) & 7u);
}

TwScan carve(void* d_scratch, uint64_t n_blocks) {
  TwScan s = {};
  const uint64_t tiles = tiles_of(n_blocks);
  s.a = static_cast<uint64_t*>(d_scratch);
  s.b = s.a + n_blocks;
  s.tiles_a = s.b + n_blocks;
  s.tiles_b = s.tiles_a + tiles + 1;
  s.err = reinterpret_cast<uint32_t*>(s.tiles_b + tiles + 1);
  s.n = n_blocks;
  s.n_tiles = tiles;
  return s;
}

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_table_write_scratch_bytes(uint64_t n_blocks, uint64_t n_tables) {
  (void)n_tables;
  // two running sums (u64) per block, each with a running sum per tile and its total; the error word
  return 8 * (2 * n_blocks + 2 * (tiles_of(n_blocks) + 1) + 1);
}

__attribute__((visibility("default"))) int lsbm_table_pack_plan_dev(
    const uint64_t* d_raw_len, const uint64_t* d_comp_len, uint64_t n_blocks, const uint64_t* d_table_block_first,
    uint64_t n_tables, const uint64_t* d_first_offset, uint64_t gap, uint8_t* d_types, uint64_t* d_handles,
    uint64_t* d_end, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (!counts_ok(n_blocks, n_tables)) return engine_fail(LSBM_ERR_INVALID, "too many blocks or tables");
  if (!d_table_block_first || (n_blocks && (!d_raw_len || !d_types || !d_handles)) ||
      (n_tables && (!d_end || !d_status)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, n_blocks, n_tables))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_table_write_scratch_bytes)");
  const Range outs[] = {{d_types, n_blocks}, {d_handles, 16 * n_blocks}, {d_end, 8 * n_tables},
                        {d_status, 4 * n_tables}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_raw_len, 8 * n_blocks}, {d_comp_len, 8 * n_blocks},
                       {d_table_block_first, 8 * (n_tables + 1)}, {d_first_offset, 8 * n_tables}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  TwPlanArgs a = {};
  a.s = carve(d_scratch, n_blocks);
  a.t = {d_table_block_first, n_tables};
  a.raw_len = d_raw_len;
  a.comp_len = d_comp_len;
  a.first_offset = d_first_offset;
  a.gap = gap;
  a.types = d_types;
  a.handles = d_handles;
  a.end = d_end;
  a.status = d_status;
  const hipError_t e = launch_table_pack_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "table pack plan kernels");
}

__attribute__((visibility("default"))) int lsbm_filter_layout_dev(
    const uint64_t* d_block_first, const uint64_t* d_table_block_first, uint64_t n_blocks, uint64_t n_tables,
    const uint64_t* d_data_handles, const uint64_t* d_data_end, int bits_per_key, uint64_t* d_filter_size,
    uint64_t* d_filter_count, uint64_t* d_filter_first, uint64_t* d_filter_out, uint64_t filters_cap, uint8_t* d_out,
    uint64_t out_size, const uint64_t* d_out_handles, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
    void* stream) {
  if (!counts_ok(n_blocks, n_tables) || filters_cap > LSBM_TABLE_WRITE_MAX_BLOCKS)
    return engine_fail(LSBM_ERR_INVALID, "too many blocks, tables or filters");
  if (bits_per_key < 0) return engine_fail(LSBM_ERR_INVALID, "bits_per_key is negative");
  if (!d_block_first || !d_table_block_first || (n_blocks && !d_data_handles) ||
      (n_tables && (!d_data_end || !d_filter_size || !d_filter_count || !d_status)) ||
      (d_out && (!d_filter_first || (filters_cap && !d_filter_out) || (n_tables && !d_out_handles))))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, n_blocks, n_tables))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_table_write_scratch_bytes)");
  const bool with = d_out != nullptr;
  const Range outs[] = {{d_filter_size, 8 * n_tables}, {d_filter_count, 8 * n_tables},
                        {d_filter_first, with ? 8 * (filters_cap + 1) : 0}, {d_filter_out, with ? 8 * filters_cap : 0},
                        {d_out, out_size}, {d_status, 4 * n_tables}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_block_first, 8 * (n_blocks + 1)}, {d_table_block_first, 8 * (n_tables + 1)},
                       {d_data_handles, 16 * n_blocks}, {d_data_end, 8 * n_tables},
                       {d_out_handles, with ? 16 * n_tables : 0}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  TwFilterArgs a = {};
  a.s = carve(d_scratch, n_blocks);
  a.t = {d_table_block_first, n_tables};
  a.block_first = d_block_first;
  a.data_handles = d_data_handles;
  a.data_end = d_data_end;
  a.bits_per_key = (uint64_t)bits_per_key;
  a.filter_size = d_filter_size;
  a.filter_count = d_filter_count;
  a.filter_first = d_filter_first;
  a.filter_out = d_filter_out;
  a.filters_cap = filters_cap;
  a.out = d_out;
  a.out_size = out_size;
  a.out_handles = d_out_handles;
  a.status = d_status;
  const hipError_t e = launch_filter_layout(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "filter layout kernels");
}

__attribute__((visibility("default"))) int lsbm_metaindex_build_dev(
    const uint64_t* d_data_end, const uint64_t* d_filter_size, uint64_t n_tables, uint64_t* d_sizes, uint8_t* d_out,
    uint64_t out_size, const uint64_t* d_out_handles, uint32_t* d_status, void* stream) {
  if (n_tables > LSBM_TABLE_WRITE_MAX_TABLES) return engine_fail(LSBM_ERR_INVALID, "too many tables");
  if (n_tables && (!d_data_end || !d_sizes || !d_status || (d_out && !d_out_handles)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const bool with = d_out != nullptr;
  const Range outs[] = {{d_sizes, 8 * n_tables}, {d_out, out_size}, {d_status, 4 * n_tables}};
  const Range ins[] = {{d_data_end, 8 * n_tables}, {d_filter_size, 8 * n_tables},
                       {d_out_handles, with ? 16 * n_tables : 0}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  TwMetaArgs a = {};
  a.data_end = d_data_end;
  a.filter_size = d_filter_size;
  a.n_tables = n_tables;
  a.sizes = d_sizes;
  a.out = d_out;
  a.out_size = out_size;
  a.out_handles = d_out_handles;
  a.status = d_status;
  const hipError_t e = launch_metaindex(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "metaindex kernel");
}

__attribute__((visibility("default"))) int lsbm_table_place_dev(
    const uint64_t* d_data_handles, uint64_t n_blocks, const uint64_t* d_table_block_first,
    const uint64_t* d_tail_handles, uint32_t tail_per_table, const uint64_t* d_tail_end, const uint64_t* d_table_base,
    uint64_t n_tables, uint8_t* d_arena, uint64_t arena_size, uint64_t* d_table_size, uint64_t* d_abs_data_handles,
    uint64_t* d_abs_tail_handles, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (!counts_ok(n_blocks, n_tables)) return engine_fail(LSBM_ERR_INVALID, "too many blocks or tables");
  if (tail_per_table != 2 && tail_per_table != 3)
    return engine_fail(LSBM_ERR_INVALID, "a table has 2 or 3 blocks after its data blocks");
  if (!d_table_block_first || (n_blocks && (!d_data_handles || !d_abs_data_handles)) || (!d_arena && arena_size) ||
      (n_tables && (!d_tail_handles || !d_tail_end || !d_table_base || !d_table_size || !d_abs_tail_handles ||
                    !d_status)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, n_blocks, n_tables))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_table_write_scratch_bytes)");
  const uint64_t n_tail = (uint64_t)tail_per_table * n_tables;
  const Range outs[] = {{d_arena, arena_size}, {d_table_size, 8 * n_tables}, {d_abs_data_handles, 16 * n_blocks},
                        {d_abs_tail_handles, 16 * n_tail}, {d_status, 4 * n_tables}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_data_handles, 16 * n_blocks}, {d_table_block_first, 8 * (n_tables + 1)},
                       {d_tail_handles, 16 * n_tail}, {d_tail_end, 8 * n_tables}, {d_table_base, 8 * n_tables}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  TwPlaceArgs a = {};
  a.t = {d_table_block_first, n_tables};
  a.err = carve(d_scratch, n_blocks).err;
  a.data_handles = d_data_handles;
  a.n = n_blocks;
  a.tail_handles = d_tail_handles;
  a.tail_per_table = tail_per_table;
  a.tail_end = d_tail_end;
  a.table_base = d_table_base;
  a.arena = d_arena;
  a.arena_size = arena_size;
  a.table_size = d_table_size;
  a.abs_data_handles = d_abs_data_handles;
  a.abs_tail_handles = d_abs_tail_handles;
  a.status = d_status;
  const hipError_t e = launch_table_place(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "table place kernels");
}

__attribute__((visibility("default"))) uint64_t lsbm_memtable_sort_segments_scratch_bytes(uint64_t n_entries,
                                                                                          uint64_t n_segs) {
  // two sets of {sort word (u64), entry (u32)} and a segment (u32) per entry; the shared prefix (u32) per
  // segment; key bytes per tile; the error word
  return 2 * 8 * n_entries + 3 * pad8(4 * n_entries) + pad8(4 * n_segs) + 8 * tiles_of(n_entries) + 8;
}

__attribute__((visibility("default"))) int lsbm_memtable_sort_segments_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries,
    const uint64_t* d_seg_first, uint64_t n_segs, uint64_t* d_source, uint64_t* d_out_key_offsets, uint64_t* d_counts,
    uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (n_entries > LSBM_MEMTABLE_MAX_ENTRIES || n_segs > LSBM_MEMTABLE_MAX_ENTRIES)
    return engine_fail(LSBM_ERR_INVALID, "too many entries or segments");
  if (!d_key_offsets || !d_seg_first || !d_out_key_offsets || !d_counts || !d_status || !d_scratch ||
      (!d_keys && keys_size) || (!d_source && n_entries))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (scratch_bytes < lsbm_memtable_sort_segments_scratch_bytes(n_entries, n_segs) ||
      (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID,
                       "scratch too small or not 8-byte aligned (lsbm_memtable_sort_segments_scratch_bytes)");
  const Range outs[] = {{d_source, 8 * n_entries}, {d_out_key_offsets, 8 * (n_entries + 1)}, {d_counts, 16},
                        {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}, {d_seg_first, 8 * (n_segs + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  SegSortArgs a = {};
  a.keys = d_keys;
  a.keys_size = keys_size;
  a.key_offsets = d_key_offsets;
  a.seg_first = d_seg_first;
  a.n = (uint32_t)n_entries;
  a.n_tiles = (uint32_t)tiles_of(n_entries);
  a.n_segs = n_segs;
  a.source = d_source;
  a.out_key_offsets = d_out_key_offsets;
  a.counts = d_counts;
  a.status = d_status;
  uint8_t* s = static_cast<uint8_t*>(d_scratch);
  a.word[0] = reinterpret_cast<uint64_t*>(s);
  a.word[1] = a.word[0] + n_entries;
  s += 16 * n_entries;
  a.index[0] = reinterpret_cast<uint32_t*>(s);
  a.index[1] = reinterpret_cast<uint32_t*>(s + pad8(4 * n_entries));
  a.seg = reinterpret_cast<uint32_t*>(s + 2 * pad8(4 * n_entries));
  s += 3 * pad8(4 * n_entries);
  a.skip = reinterpret_cast<uint32_t*>(s);
  s += pad8(4 * n_segs);
  a.tiles = reinterpret_cast<uint64_t*>(s);
  a.err = reinterpret_cast<uint32_t*>(s + 8 * tiles_of(n_entries));
  const hipError_t e = launch_sort_segments(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "segmented memtable sort kernels");
}

}  // extern "C"
