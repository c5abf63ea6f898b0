// range_types.h -- argument blocks shared by range_engine.cc (host) and
// range_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kRangeThreads = 256;  // 4 waves per workgroup
constexpr uint32_t kRangeLevels = 4;   // LSBM_RANGE_LEVELS
constexpr uint32_t kRangeCursors = 5;  // LSBM_RANGE_CURSORS
constexpr uint32_t kRangeNoRoom = 1;    // LSBM_MERGE_NO_ROOM
constexpr uint32_t kRangeBadInput = 2;  // LSBM_MERGE_BAD_INPUT

enum : uint32_t { kRsAll = 0, kRsL0Ins = 1, kRsWb = 2, kRsDel = 3, kRsCb = 4, kRsIns = 5 };
enum : uint32_t { kRangeCovers = 1, kRangeSole = 2, kRangeLast = 1 };

struct RangeKeys {  // the start and end lookup keys of n queries
  const uint8_t* start_keys;
  uint64_t start_size;
  const uint64_t* start_offsets;  // n + 1
  const uint8_t* end_keys;
  uint64_t end_size;
  const uint64_t* end_offsets;  // n + 1
  uint64_t n;
};

struct RangePlanArgs {
  const uint32_t* slot_info;  // kind | level << 8 | flags << 16
  uint64_t n_slots;
  const uint64_t* run_first;  // n_slots + 1
  uint64_t n_runs;
  const uint8_t* bounds;
  uint64_t bounds_size;
  const uint64_t* bound_offsets;  // 2 n_runs + 1
  const uint32_t* use_len;     // kRangeLevels
  const uint32_t* wb_enabled;  // kRangeLevels
  const uint8_t* cursor_keys;
  uint64_t cursor_size;
  const uint64_t* cursor_offsets;  // kRangeCursors + 1
  RangeKeys q;
  uint32_t* count;             // plan: n
  const uint64_t* pair_first;  // emit: n + 1
  uint32_t* pair_run;          // emit
  uint32_t* pair_flags;        // emit
  uint64_t pair_cap;
  uint32_t* checked;  // emit: n
  uint32_t* status;
};

struct RangeCountArgs {
  const uint8_t* index_keys;
  uint64_t index_size;
  const uint64_t* index_offsets;  // n_entries + 1
  uint64_t n_entries;
  const uint64_t* file_first;  // n_files + 1
  const uint32_t* file_state;  // n_files
  uint64_t n_files;
  RangeKeys q;
  const uint64_t* pair_first;  // n + 1
  const uint32_t* pair_file;
  const uint32_t* pair_flags;
  uint64_t n_pairs;
  uint32_t* pair_count;
  uint32_t* pair_error;
  uint32_t* found;  // n
  uint64_t* total;  // n
  uint32_t* status;
};

}  // namespace lsbm
