// memtable_types.h -- argument blocks shared by memtable_engine.cc (host) and
// memtable_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kMemThreads = 256;  // 4 waves per workgroup; the sort's tile is one workgroup's lanes
constexpr int kMemWaves = kMemThreads / 64;
constexpr uint32_t kMemTileShift = 8;  // log2(kMemThreads)

// per-record status (include/lsbm_memtable.h)
enum : uint32_t {
  kWbOk = 0, kWbTooSmall = 1, kWbBadPut = 2, kWbBadDelete = 3, kWbUnknownTag = 4, kWbWrongCount = 5,
  kWbBadInput = 6, kWbNoRoom = 7
};

struct WbArgs {
  const uint8_t* image;
  uint64_t image_size;
  const uint64_t* records;  // {offset, length} per record
  uint64_t n_records;
  // scan
  uint64_t* counts;  // {n_found, user key bytes} per record
  uint32_t* status;  // per record
  // decode
  const uint64_t* entry_base;  // n_records + 1
  const uint64_t* key_base;    // n_records + 1
  uint8_t* keys;
  uint64_t keys_cap;
  uint64_t* key_offsets;  // entries_cap + 1
  uint64_t* values;       // 2 x entries_cap
  uint64_t entries_cap;
  uint64_t* max_sequence;  // one word
};

struct MemSortArgs {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  uint32_t n;
  uint32_t n_tiles;
  uint64_t* source;           // n slots
  uint64_t* out_key_offsets;  // n + 1 slots
  uint64_t* counts;           // {n, key bytes}
  uint32_t* status;           // one word
  // scratch, carved by the engine: two ping-pong sets of {sort word, entry}
  uint64_t* word[2];
  uint32_t* index[2];
  uint64_t* tiles;  // per tile of kMemThreads sorted positions: key bytes, then their running sums
  uint32_t* err;    // nonzero once an offset or a length is bad
  uint32_t* skip;   // bytes every user key has in common at its start (the word beside err)
};

}  // namespace lsbm
