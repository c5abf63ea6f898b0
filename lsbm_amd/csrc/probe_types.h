// probe_types.h -- argument block shared by probe_engine.cc (host) and
// probe_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kProbeThreads = 256;  // 4 waves per workgroup
constexpr uint32_t kProbeLevels = 4;  // LSBM_PROBE_LEVELS
constexpr uint32_t kProbeNoRoom = 1;    // LSBM_MERGE_NO_ROOM
constexpr uint32_t kProbeBadInput = 2;  // LSBM_MERGE_BAD_INPUT

enum : uint32_t { kSlotLevel0 = 0, kSlotWb = 1, kSlotDel = 2, kSlotHead = 3, kSlotRest = 4, kSlotIns = 5 };
enum : uint32_t { kCandNone = 0, kCandMiss = 1, kCandMay = 2, kCandErr = 3 };

struct ProbeArgs {
  const uint8_t* cand;  // n_slots x n, slot-major
  uint64_t n_slots;
  const uint32_t* slot_info;  // kind | level << 8
  const uint32_t* use_len;     // kProbeLevels
  const uint32_t* wb_enabled;  // kProbeLevels
  const uint8_t* cursor_keys;
  uint64_t cursor_size;
  const uint64_t* cursor_offsets;  // kProbeLevels + 1
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  uint64_t n;
  uint32_t* count;              // plan: n
  const uint64_t* probe_first;  // emit: n + 1
  uint32_t* probe_slot;         // emit
  uint64_t probe_cap;
  uint32_t* status;
};

}  // namespace lsbm
