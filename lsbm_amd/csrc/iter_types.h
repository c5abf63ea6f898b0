// iter_types.h -- argument blocks shared by iter_engine.cc (host) and
// iter_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kIterThreads = 256;  // 4 waves per workgroup; plan's scan tile is one workgroup's lanes
constexpr int kIterWaves = kIterThreads / 64;
// what plan keeps per tile of kIterThreads positions (u64 words)
constexpr int kIterTileWords = 6;

// the call's status word (LSBM_MERGE_*: include/lsbm_block_build.h)
enum : uint32_t { kIterOk = 0, kIterNoRoom = 1, kIterBadInput = 2, kIterUnsorted = 3 };
// per-query status of a scan (include/lsbm_iter.h)
enum : uint32_t { kScanOk = 0, kScanCorruption = 1 };
// per-position flags in plan's scratch
enum : uint8_t { kFlagVisible = 1, kFlagCorrupt = 2, kFlagSegStart = 4, kFlagValue = 8 };

// the merged entries (what lsbm_merge_gather_dev writes); no value is read
struct IterEntries {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  uint64_t n;
};

struct IterPlanArgs {
  IterEntries e;
  uint64_t snapshot;
  uint64_t n_tiles;
  uint64_t* source;           // n slots: live
  uint64_t* out_key_offsets;  // n + 1 slots
  uint64_t* counts;           // {n_yield, key bytes of the live entries, corrupt entries}
  uint64_t* yield_rank;       // n + 1
  uint64_t* corrupt_rank;     // n + 1
  uint64_t* first;            // n slots, n_yield used
  int64_t* back;              // n slots, n_yield used
  uint32_t* status;           // one word
  // scratch
  uint8_t* flags;   // per position: kFlag*
  uint64_t* tiles;  // kIterTileWords per tile: partials, then running values
};

// the view a scan reads: plan's outputs, and the prefix of the live values' lengths
struct IterView {
  const uint64_t* live;              // n_yield used
  const uint64_t* live_key_offsets;  // n_yield + 1 used: internal keys, so user bytes before j = [j] - 8j
  const uint64_t* counts;            // plan's d_counts
  const uint64_t* yield_rank;        // n + 1
  const uint64_t* corrupt_rank;      // n + 1
  const uint64_t* first;
  const int64_t* back;
  const uint64_t* value_prefix;  // n_yield + 1 used
};

struct IterRangeArgs {
  IterEntries e;
  uint64_t snapshot;
  IterView v;
  const uint8_t* lo_keys;
  uint64_t lo_size;
  const uint64_t* lo_offsets;  // n_queries + 1
  const uint8_t* lo_present;   // n_queries, or null: every query has one
  const uint8_t* hi_keys;
  uint64_t hi_size;
  const uint64_t* hi_offsets;  // n_queries + 1, or null: no query has one
  const uint8_t* hi_present;   // n_queries, or null: every query has one (if hi_offsets)
  uint64_t n_queries;
  uint64_t limit;
  const uint64_t* limits;  // n_queries, or null: `limit`
  uint32_t reverse;
  uint64_t* j_begin;      // n_queries
  uint64_t* count;        // n_queries
  uint32_t* scan_status;  // n_queries: kScan*
  uint64_t* key_bytes;    // n_queries
  uint64_t* value_bytes;  // n_queries
  uint32_t* status;       // one word
};

struct IterEmitArgs {
  const uint64_t* j_begin;      // n_queries
  const uint64_t* entry_first;  // n_queries + 1: exclusive sums of count
  const uint64_t* key_first;    // n_queries + 1: of key_bytes
  const uint64_t* value_first;  // n_queries + 1: of value_bytes
  uint64_t n_queries;
  uint32_t reverse;
  const uint8_t* live_keys;  // the gathered live entries
  uint64_t live_keys_size;
  const uint64_t* live_key_offsets;  // n_live + 1
  const uint64_t* live_values;       // 2 x n_live
  uint64_t n_live;
  const uint64_t* value_prefix;  // n_live + 1
  const uint8_t* image;
  uint64_t image_size;
  uint8_t* out_keys;
  uint64_t out_keys_cap;
  uint64_t* out_key_offsets;  // entries_cap + 1
  uint8_t* out_values;
  uint64_t out_values_cap;
  uint64_t* out_value_offsets;  // entries_cap + 1
  uint64_t entries_cap;
  uint32_t* status;  // one word
};

// offsets[0..n] must not decrease, must stay within size, and every item must
// have min_len bytes or more
struct IterOffsetsArgs {
  const uint64_t* offsets;
  uint64_t n;
  uint64_t size;
  uint64_t min_len;
  uint32_t* status;
};

}  // namespace lsbm
