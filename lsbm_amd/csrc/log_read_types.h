// log_read_types.h -- argument blocks shared by log_read_engine.cc (host) and
// log_read_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kLrThreads = 256;  // 4 waves per workgroup; one scan tile is one workgroup's lanes
constexpr int kLrWaves = kLrThreads / 64;
constexpr uint32_t kLrChunk = 16;  // bytes a lane of the mover assembles and stores

// the one status word of every call (LSBM_MERGE_* of include/lsbm_block_build.h)
enum : uint32_t { kLrOk = 0, kLrNoRoom = 1, kLrBadInput = 2 };

// common/log_format.h
constexpr uint64_t kLrBlock = 32768, kLrHeader = 7;

// how a block's walk ended (d_block_end[2r]; d_block_end[2r + 1] is the bytes left)
enum : uint64_t { kEndRanOut = 0, kEndTrailer = 1, kEndBadLength = 2, kEndZeroHeader = 3, kEndTruncated = 4 };

// what a slot is to ReadRecord.  A slot is a parsed header, a block's end, or
// the end of the file: slot(header k of block r) = k + r, slot(end of block r)
// = block_first[r + 1] + r, the last slot is the end of the file.
enum : uint32_t {
  kSlotNop = 0,      // nothing: after a block's cut, a trailer, a block that ran out
  kSlotFull = 1, kSlotFirst = 2, kSlotMiddle = 3, kSlotLast = 4,
  kSlotEof = 5,      // type 5 with a good CRC, or the end of the file: the stop
  kSlotBad = 6,      // kBadRecord without a report of its own
  kSlotUnknown = 7,
  kSlotBadLength = 8, kSlotChecksum = 9,  // kBadRecord after a physical report
  kSlotTruncated = 10                     // a physical report, then nothing (the end of the file follows)
};

// the plan's scratch header (uint64 words)
enum : uint32_t { kHdrStop = 0, kHdrFrags, kHdrRecords, kHdrEvents, kHdrSide, kHdrSlots, kHdrLogBytes, kHdrInitial,
                  kHdrWords };

struct LrWalkArgs {
  const uint8_t* image;
  uint64_t log_at, log_bytes, first_block, n_blocks;
  uint64_t* block_first;  // n_blocks + 1
  uint64_t* block_end;    // 2 n_blocks
  uint64_t* headers;      // or null: count only
  uint64_t headers_cap;
  uint64_t* n_headers;
  uint32_t* status;
  uint64_t* counts;  // scratch: n_blocks + 1
  uint64_t* ends;    // scratch: 2 n_blocks
};

struct LrPlan {
  const uint8_t* image;
  uint64_t log_at, log_bytes, initial_offset, first_block, n_blocks;
  const uint64_t* block_first;
  const uint64_t* block_end;
  const uint64_t* headers;
  uint64_t n_headers;
  const uint8_t* ok;
  uint64_t* totals;
  uint32_t* status;
  uint64_t n_slots, n_tiles;
  // scratch
  uint64_t* hdr;     // kHdrWords
  uint64_t* cut;     // n_blocks: the first header of the block that fails its CRC, or block_first[r + 1]
  uint64_t* off;     // per slot: the header's offset in the log (a block's end: where the bytes left start)
  uint64_t* end;     // per slot: end_of_buffer_offset_ - buffer_.size() when ReadRecord handles it
  uint64_t* setter;  // per slot: 1 + the nearest earlier slot that sets in_fragmented_record outright, or 0
  uint64_t* mex;     // per slot: the MIDDLE lengths before it, summed
  uint64_t* scr1;    // per slot: in_fragmented_record ? 1 + scratch->size() : 0, on arrival
  uint64_t* done;    // per FIRST slot: 1 + the LAST slot that completes its record, or 0
  uint64_t* sidex;   // per slot: the side bytes before it
  uint64_t* fragex;  // per slot: the surviving fragments before it
  uint32_t* lk;      // per slot: length | kind << 16 | type byte << 24
  uint64_t* tiles;   // 6 rows of n_tiles + 1
  uint64_t* ftab;    // 3 per surviving fragment: {offset in the side area, offset in the log, length}
};

struct LrEmitArgs {
  LrPlan p;
  uint8_t* out_image;
  uint64_t side_at, side_cap;
  uint64_t* records;
  uint64_t records_cap;
  uint64_t* last_record_offset;
  uint64_t* events;
  uint64_t events_cap;
};

}  // namespace lsbm
