// include/lsbm/block_reader.h -- C++ host API for lsbm's table/ layer: a
// batched Block::Iter (table/block.cc) over host buffers.
//
// Mirrors, for many blocks of one image, what the reference does per block:
//   Block::NewIterator + SeekToFirst / Next (table/block.cc:267-270, :288-315)
//       -> ScanBlocks (counts and statuses), DecodeBlocks (keys and values)
//   Block::Iter::Seek (table/block.cc:223-265), optionally followed by
//   BlockHandle::DecodeFrom on the value (table/format.cc:23-30)
//       -> SeekBlocks
// Sits on top of the C ABI (include/lsbm_block.h); every walk runs on the GPU.
// A block is image[handles[2i], handles[2i] + handles[2i+1]).  Each call
// returns the Status of the first failing block or query in index order with
// the reference's messages: "bad block contents", "bad entry in block",
// "bad block handle".  No HIP types in this header.
#ifndef LSBM_BLOCK_READER_H_
#define LSBM_BLOCK_READER_H_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "lsbm/status.h"

namespace lsbm {

enum BlockComparator { kBytewiseComparator = 0, kInternalKeyComparator = 1 };

struct BlockCounts {
  uint64_t entries, key_bytes, value_bytes;
};

// Per block: the entries forward iteration returns before the end or the first
// error, and LSBM_BLOCK_* in (*statuses)[i].
Status ScanBlocks(int device, const char* image, size_t image_size, const uint64_t* handles, size_t n,
                  std::vector<BlockCounts>* counts, std::vector<uint32_t>* statuses);

// The entries themselves.  Block i's entries are [(*entry_first)[i],
// (*entry_first)[i+1]); entry e's key is (*keys)[(*key_offsets)[e],
// (*key_offsets)[e+1]) and its value image[(*values)[2e], + (*values)[2e+1]).
Status DecodeBlocks(int device, const char* image, size_t image_size, const uint64_t* handles, size_t n,
                    std::string* keys, std::vector<uint64_t>* key_offsets, std::vector<uint64_t>* values,
                    std::vector<uint64_t>* entry_first, std::vector<uint32_t>* statuses);

struct SeekResult {
  uint32_t state;  // LSBM_SEEK_*
  uint64_t pos, key_len, value_offset, value_size;
  uint64_t handle_offset, handle_size;  // value_is_handle
};

// Query q: Seek(targets[target_offsets[q], target_offsets[q+1])) in block
// handles[2q..2q+1].  found_keys (optional) receives the found keys.
Status SeekBlocks(int device, const char* image, size_t image_size, const uint64_t* handles,
                  const char* targets, const uint64_t* target_offsets, size_t n, BlockComparator cmp,
                  bool value_is_handle, std::vector<SeekResult>* results,
                  std::vector<std::string>* found_keys);

}  // namespace lsbm

#endif  // LSBM_BLOCK_READER_H_
