// write_types.h -- argument blocks shared by write_engine.cc (host) and
// write_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kWrThreads = 256;  // 4 waves per workgroup; the sizes' scan tile is one workgroup's lanes
constexpr int kWrWaves = kWrThreads / 64;
constexpr uint32_t kWrChainChunk = 1024;  // links (group chain) / lengths (frame plan) staged in LDS at a time
constexpr uint32_t kWrChunk = 16;         // bytes a lane of a mover assembles and stores

// the one status word of every call (LSBM_MERGE_* of include/lsbm_block_build.h)
enum : uint32_t { kWrOk = 0, kWrNoRoom = 1, kWrBadInput = 2 };

// common/log_format.h
constexpr uint64_t kLogBlock = 32768, kLogHeader = 7, kLogPayload = kLogBlock - kLogHeader;
// lsbm/db_impl.cc:1407-1410
constexpr uint64_t kGroupSmall = 128u << 10, kGroupMax = 1u << 20;

struct WrOps {
  const uint8_t* types;         // n: 1 Put, 0 Delete
  const uint8_t* keys;          // (build only)
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  const uint8_t* value_image;   // (build only)
  uint64_t value_image_size;
  const uint64_t* values;       // {offset, length} per op
  uint64_t n;
  const uint64_t* batch_first;  // n_writers + 1
  uint64_t n_writers;
};

struct WrSizesArgs {
  WrOps o;
  uint64_t* op_sum;     // n + 1
  uint64_t* batch_sum;  // n_writers + 1
  uint32_t* status;
  uint64_t* tiles;      // scratch: n_tiles + 1
  uint64_t n_tiles;
};

struct WrGroupArgs {
  const uint64_t* batch_sum;  // n + 1
  uint64_t n;                 // writers
  const uint8_t* sync;        // n, or null
  uint64_t* group_first;      // groups_cap + 1
  uint8_t* group_sync;        // groups_cap
  uint64_t groups_cap;
  uint64_t* n_groups;
  uint32_t* status;
  // scratch
  uint32_t* link;    // n: the writers a group led by w would take
  uint32_t* nsync;   // n: the first sync writer after w, or n
  uint32_t* starts;  // n: the leaders, dense
  uint64_t* count;   // their number
};

struct WrBuildArgs {
  WrOps o;
  const uint64_t* op_sum;       // n + 1
  const uint64_t* group_first;  // n_groups + 1
  uint64_t n_groups;
  uint64_t last_sequence;
  uint8_t* reps;
  uint64_t reps_cap;
  uint64_t* records;     // {offset, length} per group
  uint64_t* seq_counts;  // {sequence, count} per group
  uint64_t* new_last_sequence;
  uint32_t* status;
};

struct WrFrameArgs {
  const uint8_t* image;  // (frame only)
  uint64_t image_size;
  const uint64_t* records;  // {offset, length} per record
  uint64_t n;
  uint64_t log_offset;
  uint64_t* frag_first;  // n + 1 (plan: out; frame: in)
  uint64_t* rec_start;   // n + 1: file offset of each record's first header; slot n the end offset
  uint8_t* out;          // byte 0 is file offset log_offset
  uint64_t out_cap;
  uint64_t* headers;
  uint64_t headers_cap;
  uint32_t* status;
};

}  // namespace lsbm
