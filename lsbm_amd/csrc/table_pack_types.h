// table_pack_types.h -- argument blocks shared by table_pack_engine.cc (host)
// and table_pack_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kPackThreads = 256;  // 4 waves per workgroup; a scan tile is one workgroup's lanes
constexpr int kPackWaves = kPackThreads / 64;
// the mover's unit of work: a wave stores the kPackPieceChunks aligned 16-byte
// chunks of a piece of one block (4 KiB, 4 stores a lane); a block's last piece
// takes the one chunk more that an unaligned 4 KiB block spans
constexpr uint32_t kPackChunk = 16;
constexpr uint32_t kPackPieceChunks = 256;
constexpr uint32_t kPackMaxGrid = 2048;  // workgroups of the mover; the pieces beyond are grid-strided

// per-block status (include/lsbm_block_build.h)
enum : uint32_t { kPackOk = 0, kPackNoRoom = 1, kPackBadInput = 2 };

struct PackPlanArgs {
  const uint64_t* raw_len;   // n
  const uint64_t* comp_len;  // n, or null: every block stays raw
  uint64_t n;
  uint64_t n_tiles;
  uint64_t first_offset;
  uint64_t gap;
  uint8_t* types;     // n
  uint64_t* handles;  // 2n
  uint64_t* end;      // one slot
  uint64_t* tiles;    // scratch: n_tiles + 1 running sums
};

struct PackArgs {
  const uint8_t* raw;
  uint64_t raw_size;
  const uint64_t* raw_handles;  // 2n; only the offsets are read
  const uint8_t* comp;
  uint64_t comp_size;
  const uint64_t* comp_offsets;  // n
  const uint8_t* types;          // n
  const uint64_t* handles;       // 2n
  uint64_t n;
  uint64_t n_tiles;
  uint64_t gap;
  uint8_t* out;
  uint64_t out_size;
  uint32_t* status;   // n
  uint64_t* pieces;   // scratch: per block, the pieces of the blocks before it in its tile
  uint64_t* tiles;    // scratch: n_tiles + 1 running sums of the tiles' pieces
};

}  // namespace lsbm
