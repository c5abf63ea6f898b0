// block_build_types.h -- argument blocks shared by block_build_engine.cc (host)
// and block_build_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kBuildThreads = 256;  // 4 waves per workgroup, one block (or table) per wave
constexpr int kBuildWaves = kBuildThreads / 64;
// A wave's LDS tile: a block of at most this size is assembled there and
// stored with aligned 16-B stores; a larger one is written straight to global
// memory by the same code.  + 16: the tile keeps the window's 16-B phase.
constexpr uint32_t kBuildTileBytes = 8192;
constexpr uint32_t kBuildTileAlloc = kBuildTileBytes + 16;
// plan's chain: links staged in LDS, this many at a time
constexpr uint32_t kPlanChunk = 1024;

// per-block / per-table status (include/lsbm_block_build.h)
enum : uint32_t { kBuildOk = 0, kBuildNoRoom = 1, kBuildBadInput = 2, kBuildTooLarge = 3 };

// the entries (what lsbm_block_decode_dev writes)
struct BuildEntries {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  const uint64_t* values;       // {offset, length} per entry
  const uint8_t* value_image;   // not read by plan
  uint64_t value_image_size;
  uint64_t n;
};

// plan's scratch, carved by the engine
struct PlanScratch {
  uint32_t* sizes;     // 2 per entry: encoded size with the shared prefix, and as a restart point (saturating)
  uint64_t* link;      // per entry: entries of the block that starts here (>= 1), tables ignored
  uint64_t* bytes;     // per entry: Finish() size of that block
  uint64_t* starts;    // table t's block starts at [table_first[t], ...)
  uint64_t* counts;    // per table: blocks
  uint64_t* last;      // per table: Finish() size of its last block
};

struct PlanArgs {
  BuildEntries e;
  const uint64_t* table_first;  // n_tables + 1
  uint64_t n_tables;
  uint64_t block_size;
  uint32_t restart_interval;
  uint64_t* block_first;        // blocks_cap + 1
  uint64_t* block_bytes;        // blocks_cap
  uint64_t blocks_cap;
  uint64_t* table_block_first;  // n_tables + 1
  uint32_t* status;             // per table
  PlanScratch s;
};

struct BuildArgs {
  BuildEntries e;
  const uint64_t* block_first;  // n_blocks + 1
  uint64_t n_blocks;
  uint32_t restart_interval;
  uint8_t* out;
  uint64_t out_size;
  const uint64_t* out_handles;  // {offset, size} window per block
  uint64_t* built_bytes;        // nullable
  uint32_t* status;
};

struct IndexArgs {
  BuildEntries e;               // keys only
  const uint64_t* block_first;  // n_blocks + 1
  uint64_t n_blocks;
  const uint64_t* table_block_first;  // n_tables + 1
  uint64_t n_tables;
  const uint64_t* data_handles;  // {offset, size} per data block
  uint32_t cmp;
  uint8_t* out;                  // nullable: sizes only
  uint64_t out_size;
  const uint64_t* out_handles;   // {offset, size} window per table
  uint64_t* built_bytes;
  uint32_t* status;
};

}  // namespace lsbm
