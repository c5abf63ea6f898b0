// merge_types.h -- argument blocks shared by merge_engine.cc (host) and
// merge_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kMergeThreads = 256;  // 4 waves per workgroup; select's scan tile is one workgroup's lanes
constexpr int kMergeWaves = kMergeThreads / 64;
constexpr uint32_t kMergeMaxRuns = 64;
// rank's first level: every kMergeSample-th entry of a run searches the other
// runs whole and keeps its bounds; the entries between two samples search only
// between the two samples' bounds
constexpr uint32_t kMergeSample = 64;

// per-run status (include/lsbm_merge.h)
enum : uint32_t { kMergeOk = 0, kMergeNoRoom = 1, kMergeBadInput = 2, kMergeUnsorted = 3 };
// flags (include/lsbm_merge.h)
enum : uint32_t { kMergeDrop = 1, kMergeBottomLevel = 2 };

// the input entries (what lsbm_block_decode_dev writes); values are not read by plan
struct MergeEntries {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  const uint64_t* values;       // {offset, length} per entry
  uint64_t n;
};

// plan's scratch, carved by the engine
struct MergeScratch {
  uint64_t* order;  // per merged position: the input entry there
  uint32_t* keep;   // per merged position: 1 if the entry survives the drop rule
  uint64_t* tiles;  // per tile of kMergeThreads positions: {kept entries, kept key bytes}, then their running sums
  uint32_t* err;    // nonzero once any run is in error
  uint64_t* bounds;  // per sample slot and run: the sample's bound in that run (an entry index)
  uint64_t n_slots;  // sample i of run r has slot run_first[r] / kMergeSample + r + i
};

struct MergePlanArgs {
  MergeEntries e;
  const uint64_t* run_first;  // n_runs + 1
  uint32_t n_runs;
  uint32_t cmp;
  uint32_t flags;
  uint64_t smallest_snapshot;
  uint64_t n_tiles;
  uint64_t* source;           // n slots
  uint64_t* out_key_offsets;  // n + 1 slots
  uint64_t* counts;           // {n_out, key bytes of the output}
  uint32_t* run_status;       // per run
  MergeScratch s;
};

struct MergeGatherArgs {
  MergeEntries e;
  const uint64_t* source;            // n slots, n_out used
  const uint64_t* plan_key_offsets;  // n + 1 slots, n_out + 1 used
  const uint64_t* counts;
  uint8_t* out_keys;
  uint64_t out_keys_cap;
  uint64_t* out_key_offsets;  // entries_cap + 1
  uint64_t* out_values;       // 2 x entries_cap
  uint64_t entries_cap;
  uint32_t* status;           // one word
};

}  // namespace lsbm
