// memtable_engine.cc -- the device entry points of include/lsbm_memtable.h.
//
// Validates arguments, carves the sort's scratch and launches
// memtable_kernels.hip on the caller's stream.  Never walks or sorts on the
// CPU: without a usable device every entry point returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_memtable.h"
#include "engine_internal.h"
#include "memtable_types.h"

namespace lsbm {

// launchers (memtable_kernels.hip)
hipError_t launch_wb_scan(const WbArgs& a, hipStream_t stream);
hipError_t launch_wb_decode(const WbArgs& a, hipStream_t stream);
hipError_t launch_memtable_sort(const MemSortArgs& a, hipStream_t stream);

namespace {

constexpr uint64_t kMaxRecords = 1ull << 36;

uint64_t tiles_of(uint64_t n) { return (n + kMemThreads - 1) / kMemThreads; }
uint64_t pad8(uint64_t bytes) { return (bytes + 7) & ~7ull; }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) int lsbm_wb_scan_dev(const uint8_t* d_image, uint64_t image_size,
                                                            const uint64_t* d_records, uint64_t n_records,
                                                            uint64_t* d_counts, uint32_t* d_status, void* stream) {
  if (n_records > kMaxRecords) return engine_fail(LSBM_ERR_INVALID, "too many records");
  if ((!d_image && image_size) || (n_records && (!d_records || !d_counts || !d_status)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_counts, 16 * n_records}, {d_status, 4 * n_records}};
  const Range ins[] = {{d_image, image_size}, {d_records, 16 * n_records}};
  if (any_overlap(outs, ins) || overlap(d_counts, 16 * n_records, d_status, 4 * n_records))
    return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WbArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.records = d_records;
  a.n_records = n_records;
  a.counts = d_counts;
  a.status = d_status;
  const hipError_t e = launch_wb_scan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "wb_scan_kernel");
}

__attribute__((visibility("default"))) int lsbm_wb_decode_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n_records,
    const uint64_t* d_entry_base, const uint64_t* d_key_base, uint8_t* d_keys, uint64_t keys_cap,
    uint64_t* d_key_offsets, uint64_t* d_values, uint64_t entries_cap, uint64_t* d_max_sequence, uint32_t* d_status,
    void* stream) {
  if (n_records > kMaxRecords || entries_cap > kMaxRecords) return engine_fail(LSBM_ERR_INVALID, "too many records");
  if ((!d_image && image_size) || !d_entry_base || !d_key_base || !d_key_offsets || !d_max_sequence ||
      (!d_keys && keys_cap) || (!d_values && entries_cap) || (n_records && (!d_records || !d_status)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_keys, keys_cap}, {d_key_offsets, 8 * (entries_cap + 1)}, {d_values, 16 * entries_cap},
                        {d_max_sequence, 8}, {d_status, 4 * n_records}};
  const Range ins[] = {{d_image, image_size}, {d_records, 16 * n_records}, {d_entry_base, 8 * (n_records + 1)},
                       {d_key_base, 8 * (n_records + 1)}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  for (size_t i = 0; i < 5; i++)
    for (size_t j = i + 1; j < 5; j++)
      if (overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n))
        return engine_fail(LSBM_ERR_INVALID, "outputs alias each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  WbArgs a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.records = d_records;
  a.n_records = n_records;
  a.status = d_status;
  a.entry_base = d_entry_base;
  a.key_base = d_key_base;
  a.keys = d_keys;
  a.keys_cap = keys_cap;
  a.key_offsets = d_key_offsets;
  a.values = d_values;
  a.entries_cap = entries_cap;
  a.max_sequence = d_max_sequence;
  const hipError_t e = launch_wb_decode(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "wb_decode_kernel");
}

__attribute__((visibility("default"))) uint64_t lsbm_memtable_sort_scratch_bytes(uint64_t n_entries) {
  // two sets of {sort word (u64), entry (u32)} per entry; key bytes per tile; the error word and the shared prefix
  return 2 * 8 * n_entries + 2 * pad8(4 * n_entries) + 8 * tiles_of(n_entries) + 8;
}

__attribute__((visibility("default"))) int lsbm_memtable_sort_dev(
    const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_entries, uint64_t* d_source,
    uint64_t* d_out_key_offsets, uint64_t* d_counts, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
    void* stream) {
  if (n_entries > LSBM_MEMTABLE_MAX_ENTRIES) return engine_fail(LSBM_ERR_INVALID, "too many entries");
  if (!d_key_offsets || !d_out_key_offsets || !d_counts || !d_status || !d_scratch || (!d_keys && keys_size) ||
      (!d_source && n_entries))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (scratch_bytes < lsbm_memtable_sort_scratch_bytes(n_entries) || (reinterpret_cast<uint64_t>(d_scratch) & 7u))
    return engine_fail(LSBM_ERR_INVALID,
                       "scratch too small or not 8-byte aligned (lsbm_memtable_sort_scratch_bytes)");
  const Range outs[] = {{d_source, 8 * n_entries}, {d_out_key_offsets, 8 * (n_entries + 1)}, {d_counts, 16},
                        {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_keys, keys_size}, {d_key_offsets, 8 * (n_entries + 1)}};
  if (any_overlap(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  for (size_t i = 0; i < 5; i++)
    for (size_t j = i + 1; j < 5; j++)
      if (overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n))
        return engine_fail(LSBM_ERR_INVALID, "outputs alias each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MemSortArgs a = {};
  a.keys = d_keys;
  a.keys_size = keys_size;
  a.key_offsets = d_key_offsets;
  a.n = (uint32_t)n_entries;
  a.n_tiles = (uint32_t)tiles_of(n_entries);
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
  s += 2 * pad8(4 * n_entries);
  a.tiles = reinterpret_cast<uint64_t*>(s);
  a.err = reinterpret_cast<uint32_t*>(s + 8 * tiles_of(n_entries));
  a.skip = a.err + 1;
  const hipError_t e = launch_memtable_sort(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "memtable sort kernels");
}

}  // extern "C"
