// block_types.h -- argument blocks shared by block_engine.cc (host) and
// block_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kBlockThreads = 256;  // 4 waves per workgroup
constexpr int kBlockWaves = kBlockThreads / 64;
// A wave's LDS tile: blocks up to this size are staged (a 4 KiB-class data
// block with its restart array); larger ones (index blocks) are walked from
// global memory by the same code.  + 32: the block keeps its 16-B phase.
constexpr uint32_t kBlockTileBytes = 8192;
constexpr uint32_t kBlockTileAlloc = kBlockTileBytes + 32;

// scan / decode status per block (include/lsbm_block.h)
enum : uint32_t { kBlkOk = 0, kBlkBadContents = 1, kBlkBadEntry = 2, kBlkNoRoom = 3 };
// seek state per query
enum : uint32_t { kSeekValid = 0, kSeekNotValid = 1, kSeekBadEntry = 2, kSeekBadContents = 3, kSeekBadHandle = 4 };

struct BlockWalkArgs {
  const uint8_t* image;
  uint64_t image_size;
  const uint64_t* handles;  // {offset, size} per block
  uint64_t n;
  uint64_t* counts;         // {entries, key bytes, value bytes} per block (nullable in decode)
  uint32_t* status;
  // decode only
  const uint64_t* entry_base;  // n + 1: block b's entries [entry_base[b], entry_base[b+1])
  const uint64_t* key_base;    // n + 1: block b's key bytes [key_base[b], key_base[b+1])
  uint8_t* keys;
  uint64_t keys_cap;
  uint64_t* key_offsets;       // entries_cap + 1
  uint64_t* values;            // 2 * entries_cap
  uint64_t entries_cap;
};

struct BlockSeekArgs {
  const uint8_t* image;
  uint64_t image_size;
  const uint64_t* handles;  // {offset, size} per query
  const uint8_t* keys;      // targets
  const uint64_t* key_offsets;
  uint64_t n;
  uint32_t cmp;
  uint32_t flags;
  uint32_t* state;
  uint64_t* pos;
  uint64_t* key_len;
  uint64_t* value;          // {absolute offset, length} per query
  uint64_t* handle_out;     // {offset, size} per query (LSBM_SEEK_VALUE_IS_HANDLE)
  uint8_t* found;           // nullable
  const uint64_t* found_offsets;  // n + 1
  uint64_t found_cap;
};

}  // namespace lsbm
