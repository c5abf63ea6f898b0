// include/lsbm/block_builder.h -- C++ host API for lsbm's table/ layer: a
// batched BlockBuilder (table/block_builder.cc) with TableBuilder's flush rule
// and index block (table/table_builder.cc), over host buffers.
//
// Mirrors, for many blocks at once, what the reference does per key:
//   TableBuilder::Add's "flush when CurrentSizeEstimate() >= block_size"
//   (table/table_builder.cc:137-140)                  -> PlanBlocks
//   BlockBuilder::Add / Finish (table/block_builder.cc:57-107) -> BuildBlocks
//   the index entries: FindShortestSeparator / FindShortSuccessor and
//   BlockHandle::EncodeTo (table/table_builder.cc:120-127, :292-299)
//                                                     -> BuildIndexBlocks
// Sits on top of the C ABI (include/lsbm_block_build.h); every block is built
// on the GPU.  Entries are what DecodeBlocks (include/lsbm/block_reader.h)
// returns: entry e's key is keys[key_offsets[e], key_offsets[e+1]) and its
// value value_image[values[2e], + values[2e+1]).  Each call returns the Status
// of the first failing block or table in index order: InvalidArgument for
// bad input and for a block that would reach 2^32 bytes.  No HIP types in
// this header.
#ifndef LSBM_BLOCK_BUILDER_H_
#define LSBM_BLOCK_BUILDER_H_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "lsbm/block_reader.h"  // BlockComparator
#include "lsbm/status.h"

namespace lsbm {

struct BlockEntries {
  const char* keys;
  size_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  const uint64_t* values;       // {offset, length} per entry
  const char* value_image;      // not read by PlanBlocks and BuildIndexBlocks
  size_t value_image_size;
  size_t n;
};

// Table t owns entries [table_first[t], table_first[t+1]).  Block b holds
// entries [(*block_first)[b], (*block_first)[b+1]) and Finish() will return
// (*block_bytes)[b] bytes; table t's blocks are [(*table_block_first)[t],
// (*table_block_first)[t+1]).  (*statuses)[t]: LSBM_BUILD_*.
Status PlanBlocks(int device, const BlockEntries& entries, const uint64_t* table_first, size_t n_tables,
                  uint64_t block_size, uint32_t restart_interval, std::vector<uint64_t>* block_first,
                  std::vector<uint64_t>* block_bytes, std::vector<uint64_t>* table_block_first,
                  std::vector<uint32_t>* statuses);

// The blocks' contents back to back in *out: block b is
// (*out)[(*block_offsets)[b], (*block_offsets)[b+1]).  A block in error is
// empty.  (*statuses)[b]: LSBM_BUILD_*.
Status BuildBlocks(int device, const BlockEntries& entries, const uint64_t* block_first, size_t n_blocks,
                   uint32_t restart_interval, std::string* out, std::vector<uint64_t>* block_offsets,
                   std::vector<uint32_t>* statuses);

// One index block per table, back to back in *out as above.  data_handles:
// {offset, size} of every data block in its file.
Status BuildIndexBlocks(int device, const BlockEntries& entries, const uint64_t* block_first, size_t n_blocks,
                        const uint64_t* table_block_first, size_t n_tables, const uint64_t* data_handles,
                        BlockComparator cmp, std::string* out, std::vector<uint64_t>* block_offsets,
                        std::vector<uint32_t>* statuses);

}  // namespace lsbm

#endif  // LSBM_BLOCK_BUILDER_H_
