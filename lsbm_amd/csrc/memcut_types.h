// memcut_types.h -- argument blocks shared by memcut_engine.cc (host) and
// memcut_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kMcThreads = 256;  // 4 waves per workgroup
constexpr int kMcWave = 64;      // the walk is one wave of a workgroup
constexpr uint32_t kMcChunk = 4096;  // slots the walk's workgroup stages in LDS at a time
constexpr uint32_t kMcDraws = 64;                       // generator draws a lane walks
constexpr uint32_t kMcWgDraws = kMcThreads * kMcDraws;  // and a workgroup: 16,384

// the one status word of a cut (LSBM_MERGE_* of include/lsbm_block_build.h)
enum : uint32_t { kMcOk = 0, kMcNoRoom = 1, kMcBadInput = 2 };
enum : uint32_t { kMcRecover = 0, kMcWrite = 1 };

// util/random.h, common/skiplist.h, util/arena.cc, common/memtable.cc
constexpr uint64_t kMcM = 2147483647ull, kMcA = 16807ull, kMcSeed = 0xdeadbeefull & 0x7fffffffull;
constexpr uint32_t kMcMaxHeight = 12;  // kBranching 4: a draw succeeds when x % 4 == 0
constexpr uint64_t kMcBlock = 4096, kMcHeadNode = 8 + 8 * kMcMaxHeight, kMcFresh = kMcBlock + 8;

// What a range of consecutive draws does to the height loop, whatever state
// (successes so far in the current insert, 0..10) it is entered with: `lead`
// successes, then (lead < len) a failure, then `rest` further inserts
// completed, and `tail` successes pending at the end.
struct McRun {
  uint32_t lead, rest, tail, len;
};

struct McHeightsArgs {
  uint64_t rnd;           // the generator state before the first draw ...
  const uint64_t* d_rnd;  // ... or where it lies in device memory
  uint64_t n, n_wgs;
  uint8_t* heights;     // n
  uint32_t* rnd_after;  // n, or null: the state after each insert
  uint64_t* rnd_out;    // or null: the state after the n-th
  McRun* runs;          // scratch: n_wgs
  uint64_t* link;       // scratch: 2 n_wgs {inserts before the workgroup's draws, pending successes}
};

// a slot is an entry or a record's test point: record i's slots start at
// entry_base[i] + i; RECOVER puts the test after the entries, WRITE before
enum : uint64_t { kSlotDead = 0, kSlotEntry = 1, kSlotTest = 2 };
constexpr uint32_t kSlotKindShift = 40;  // the word: L | kind << 40

// the walk's results in the scratch (uint64 words)
enum : uint32_t { kMcState = 0, kMcMems = 6, kMcContinues = 7, kMcHdrWords = 8 };

struct McCutArgs {
  const uint64_t* key_offsets;
  uint64_t key_extra;
  const uint64_t* values;
  const uint8_t* types;  // or null
  const uint64_t* entry_base;
  const uint32_t* rec_status;  // or null
  uint64_t n_entries, n_records, n_slots;
  uint32_t mode;
  uint32_t one_lane;  // the walk by one lane (mc_walk_lane_kernel) instead of the wave
  uint64_t write_buffer_size;
  const uint64_t* state_in;  // or null
  uint64_t* usage;
  uint64_t* mem_first;
  uint64_t* mem_usage;
  uint64_t mem_cap;
  uint64_t* counts;
  uint64_t* state_out;
  uint32_t* status;
  // scratch
  uint64_t* hdr;       // kMcHdrWords
  uint64_t* words;     // per slot
  uint64_t* uout;      // per slot: ApproximateMemoryUsage() after it
  uint64_t* mem_slot;  // n_records + 1: the slot that created (or joined) each memtable
  uint64_t* mem_use;   // n_records + 1
  const uint8_t* h0;   // heights from the fixed seed, n_entries
  const uint32_t* r0;
  const uint8_t* h1;  // heights from state_in's generator state, n_entries (null without state_in)
  const uint32_t* r1;
};

}  // namespace lsbm
