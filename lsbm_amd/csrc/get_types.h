// get_types.h -- argument blocks shared by get_engine.cc (host) and
// get_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kGetThreads = 256;     // 4 waves per workgroup
constexpr int kGatherLanes = 16;     // lanes that copy one value in slices_gather_kernel
constexpr uint32_t kGetBadInput = 2;  // LSBM_MERGE_BAD_INPUT

// per-query verdict (include/lsbm_get.h)
enum : uint32_t { kGetUndecided = 0, kGetFound = 1, kGetDeleted = 2, kGetCorrupt = 3, kGetError = 16 };
// table-read states
enum : uint32_t { kStateValid = 0, kStateNotValid = 1, kStateFiltered = 6, kStateMax = 15 };
enum : uint32_t { kRunLevel0 = 1 };

// offsets[0..n] must not decrease, must stay within size, and every key must
// have min_len bytes or more
struct OffsetsArgs {
  const uint64_t* offsets;
  uint64_t n;
  uint64_t size;
  uint64_t min_len;
  uint32_t* status;
};

struct LookupArgs {
  const uint8_t* user_keys;
  uint64_t user_size;
  const uint64_t* user_offsets;  // n + 1
  uint64_t n;
  uint64_t snapshot;
  const uint64_t* snapshots;  // n, or null
  uint8_t* keys;
  uint64_t keys_cap;
  uint64_t* key_offsets;  // n + 1
  uint32_t* status;
};

// the lookup keys and the per-query outputs every probe shares
struct QueryArgs {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  uint64_t n;
  int32_t source_id;
  uint32_t* verdict;
  uint64_t* value;  // 2 x n
  int32_t* where;
  uint32_t* status;
};

struct MemGetArgs {
  QueryArgs q;
  const uint8_t* mem_keys;
  uint64_t mem_keys_size;
  const uint64_t* mem_key_offsets;  // n_entries + 1
  const uint64_t* mem_values;       // 2 x n_entries
  uint64_t n_entries;
};

struct FindFileArgs {
  const uint8_t* bounds;
  uint64_t bounds_size;
  const uint64_t* bound_offsets;  // 2 x n_files + 1
  uint64_t n_files;
  const uint64_t* run_first;  // n_runs + 1
  const uint32_t* run_flags;  // n_runs
  const uint8_t* visible;     // n_files
  uint64_t n_runs;
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;
  uint64_t n;
  int32_t* file;  // n x n_runs
  uint32_t* status;
};

struct SaveArgs {
  QueryArgs q;
  const uint32_t* state;
  const uint64_t* key_len;
  const uint8_t* found;
  uint64_t found_size;
  const uint64_t* found_offsets;  // n + 1
  const uint64_t* value_in;       // 2 x n
};

struct GatherArgs {
  const uint8_t* image;
  uint64_t image_size;
  const uint64_t* slices;  // 2 x n
  const int32_t* where;
  int32_t where_lo, where_hi;
  uint8_t* out;
  uint64_t out_cap;
  const uint64_t* out_offsets;  // n + 1
  uint64_t n;
  uint32_t* status;
};

}  // namespace lsbm
