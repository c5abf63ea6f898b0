// memtable_flush_host.h -- the part of memtable_flush.cc that does not touch
// the device: the records' staging layout, the status mapping, the filter
// block's layout and the small blocks TableBuilder::Finish writes itself.
// Plain C++ (memtable_flush_host.cc), so that it also builds into a stand-alone
// program under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/lsbm/status.h"

namespace lsbm {
namespace level0 {

// The records back to back: record i is image[pairs[2i], + pairs[2i+1]).
// Returns the image's size.
uint64_t LayoutRecords(const std::vector<std::string>& records, std::vector<uint64_t>* pairs);

// LSBM_WB_* -> the Status the reference returns for the record
// (common/write_batch.cc:42-80, lsbm/db_impl.cc:440-443).
Status RecordStatus(uint32_t wb_status, size_t record);

// The running sums lsbm_wb_decode_dev takes, from lsbm_wb_scan_dev's counts
// ({entries, user-key bytes} per record): n + 1 slots each.
void Bases(const uint64_t* counts, size_t n_records, std::vector<uint64_t>* entry_base,
           std::vector<uint64_t>* key_base);

void PutVarint64(std::string* dst, uint64_t v);

// FilterBlockBuilder (table/filter_block.cc:22-76) over data blocks that start
// at file offsets block_start[b] and hold keys [block_first[b], block_first[b+1]);
// `end` is the offset after the last data block (the last StartBlock).
// Filter f holds keys [filter_first[f], filter_first[f+1]) and goes to
// filter_out[f] of the block; *trailer is the offset array, its offset and
// kFilterBaseLg, which follow the data_bytes of filters.
struct FilterLayout {
  std::vector<uint64_t> filter_first;  // n_filters + 1 (empty without a filter)
  std::vector<uint64_t> filter_out;    // n_filters
  uint64_t data_bytes = 0;
  std::string trailer;
};
void LayoutFilterBlock(const uint64_t* block_start, const uint64_t* block_first, size_t n_blocks, uint64_t end,
                       int bits_per_key, FilterLayout* out);

// The metaindex block: one entry "filter.<policy name>" -> the filter block's
// handle when there is a filter, else an empty block
// (table/table_builder.cc:269-284).
std::string MetaindexBlock(bool with_filter, uint64_t filter_offset, uint64_t filter_size);

// Footer::EncodeTo (table/format.cc:32-42).
std::string Footer(uint64_t meta_offset, uint64_t meta_size, uint64_t index_offset, uint64_t index_size);

}  // namespace level0
}  // namespace lsbm
