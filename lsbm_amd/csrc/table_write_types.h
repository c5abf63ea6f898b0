// table_write_types.h -- argument blocks shared by table_write_engine.cc (host)
// and table_write_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kTwThreads = 256;  // 4 waves per workgroup; a scan tile and a sort tile are one workgroup's lanes
constexpr int kTwWaves = kTwThreads / 64;
constexpr uint32_t kTwFilterBaseLg = 11;  // table/filter_block.cc:15
constexpr uint64_t kTwFooterBytes = 48;   // table/format.h:70
constexpr uint64_t kTwNoPlace = ~0ull;    // LSBM_TABLE_NO_PLACE

// per-table status (include/lsbm_block_build.h)
enum : uint32_t { kTwOk = 0, kTwNoRoom = 1, kTwBadInput = 2 };

// Running sums over the blocks of a call, in scratch: a[i] / b[i] are block
// i's sums inside its tile of kTwThreads blocks, tiles_a / tiles_b the sums of
// the tiles before a tile, their slot n_tiles the sum of all.
struct TwScan {
  uint64_t* a;        // n
  uint64_t* b;        // n (the filter layout only)
  uint64_t* tiles_a;  // n_tiles + 1
  uint64_t* tiles_b;  // n_tiles + 1
  uint32_t* err;      // nonzero: table_block_first does not tile the blocks
  uint64_t n;
  uint64_t n_tiles;
};

struct TwTables {
  const uint64_t* table_block_first;  // n_tables + 1
  uint64_t n_tables;
};

struct TwPlanArgs {
  TwScan s;
  TwTables t;
  const uint64_t* raw_len;       // n
  const uint64_t* comp_len;      // n, or null: every block stays raw
  const uint64_t* first_offset;  // n_tables, or null: 0
  uint64_t gap;
  uint8_t* types;     // n
  uint64_t* handles;  // 2n
  uint64_t* end;      // n_tables
  uint32_t* status;   // n_tables
};

struct TwFilterArgs {
  TwScan s;
  TwTables t;
  const uint64_t* block_first;   // n + 1
  const uint64_t* data_handles;  // 2n, relative
  const uint64_t* data_end;      // n_tables
  uint64_t bits_per_key;
  uint64_t* filter_size;   // n_tables
  uint64_t* filter_count;  // n_tables
  uint64_t* filter_first;  // filters_cap + 1 (with out)
  uint64_t* filter_out;    // filters_cap
  uint64_t filters_cap;
  uint8_t* out;  // null: sizes only
  uint64_t out_size;
  const uint64_t* out_handles;  // 2 n_tables
  uint32_t* status;             // n_tables
};

struct TwMetaArgs {
  const uint64_t* data_end;
  const uint64_t* filter_size;  // null: the empty block
  uint64_t n_tables;
  uint64_t* sizes;
  uint8_t* out;  // null: sizes only
  uint64_t out_size;
  const uint64_t* out_handles;
  uint32_t* status;
};

struct TwPlaceArgs {
  TwTables t;
  uint32_t* err;
  const uint64_t* data_handles;  // 2n
  uint64_t n;
  const uint64_t* tail_handles;  // 2 x tail_per_table x n_tables
  uint32_t tail_per_table;
  const uint64_t* tail_end;
  const uint64_t* table_base;
  uint8_t* arena;
  uint64_t arena_size;
  uint64_t* table_size;
  uint64_t* abs_data_handles;
  uint64_t* abs_tail_handles;
  uint32_t* status;
};

struct SegSortArgs {
  const uint8_t* keys;
  uint64_t keys_size;
  const uint64_t* key_offsets;  // n + 1
  const uint64_t* seg_first;    // n_segs + 1
  uint32_t n;
  uint32_t n_tiles;
  uint64_t n_segs;
  uint64_t* source;           // n slots
  uint64_t* out_key_offsets;  // n + 1 slots
  uint64_t* counts;           // {n, key bytes}
  uint32_t* status;           // one word
  // scratch, carved by the engine: two ping-pong sets of {sort word, entry}
  uint64_t* word[2];
  uint32_t* index[2];
  uint32_t* seg;    // per entry: its segment
  uint32_t* skip;   // per segment: bytes every user key of it has in common at its start
  uint64_t* tiles;  // per tile of kTwThreads sorted positions: key bytes, then their running sums
  uint32_t* err;    // nonzero once an offset, a length or seg_first is bad
};

}  // namespace lsbm
