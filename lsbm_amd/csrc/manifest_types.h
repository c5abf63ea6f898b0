// manifest_types.h -- argument blocks shared by manifest_engine.cc (host) and
// manifest_kernels.hip (device).  Plain C++, no HIP headers.
#pragma once
#include <stdint.h>

namespace lsbm {

constexpr int kMfThreads = 256;  // 4 waves per workgroup; one scan tile is one workgroup's lanes
constexpr int kMfWaves = kMfThreads / 64;

// the one status word of every call (LSBM_MERGE_* of include/lsbm_block_build.h)
enum : uint32_t { kMfOk = 0, kMfNoRoom = 1, kMfBadInput = 2 };

// lsbm/version_edit.cc:14-26
enum : uint32_t { kTagComparator = 1, kTagLogNumber = 2, kTagNextFile = 3, kTagLastSequence = 4, kTagDeletedFile = 6,
                  kTagNewFile = 7, kTagPrevLogNumber = 9, kTagWriteCursor = 10, kTagReadCursor = 11 };
constexpr uint32_t kMfLevels = 4;  // config::kNumLevels, include/leveldb/params.h:55
constexpr uint32_t kMfTypes = 4;   // deleted_files_[4], new_files_[4]

// a record's verdict: 0, the reference's eleven messages, the two library codes
enum : uint32_t { kVerOk = 0, kVerComparator, kVerLogNumber, kVerPrevLogNumber, kVerNextFile, kVerLastSequence,
                  kVerDeletedFile, kVerNewFile, kVerWriteCursor, kVerReadCursor, kVerUnknownTag, kVerInvalidTag,
                  kVerTypeRange, kVerCursorRange };

// the words of an edit's fields (LSBM_EDIT_* of include/lsbm_manifest.h)
enum : uint32_t { kFHas = 0, kFReadHas, kFLog, kFPrevLog, kFNextFile, kFLastSeq, kFWriteCursor, kFRead0,
                  kFCmpOff = kFRead0 + 4, kFCmpLen, kMfFieldWords };
// a field's slot is its bit in kFHas (0..5) or 6 + i for read cursor i
constexpr uint32_t kMfSlots = 10;
constexpr uint32_t kNewWords = 5, kDelWords = 4;  // {record, type, level, number[, file_size]}

// the scratch header (uint64 words) a plan leaves for its second call
enum : uint32_t { kMhN = 0, kMhSpan, kMhNew, kMhDel, kMhKeyBytes, kMhBytes, kMhWords = 8 };

struct MfDecode {
  const uint8_t* image;
  uint64_t image_size;
  const uint64_t* records;  // 2 n: {offset, length}
  uint64_t n, span_cap, longest_cap, n_tiles;
  uint32_t rounds;
  // the first call's outputs
  uint32_t* verdict;    // n
  uint64_t* fields;     // kMfFieldWords n
  uint64_t* new_first;  // n + 1
  uint64_t* del_first;  // n + 1
  uint64_t* totals;     // 3: {n_new, n_deleted, key bytes}
  uint32_t* status;
  // the second call's outputs
  uint64_t* new_items;
  uint64_t new_cap;
  uint64_t* key_offsets;  // 2 new_cap + 1
  uint8_t* keys;
  uint64_t keys_cap;
  uint64_t* del_items;
  uint64_t del_cap;
  // scratch
  uint64_t* hdr;        // kMhWords
  uint64_t* rec_first;  // n + 1: the records' lengths, summed; a position is a byte of the records laid end to end
  uint64_t* win;        // kMfSlots n: 1 + the last position that sets the slot
  uint64_t* tiles;      // 3 rows of n_tiles + 1: new files, deleted files, key bytes
  uint32_t* ver;        // n
  uint32_t* nxt_a;      // span_cap: where the group that begins at a position ends, or span + verdict
  uint32_t* nxt_b;
  uint8_t* kind;        // span_cap: the tag of a group that parses | 0x80 reachable; after the plan: the tag of a live item
};

struct MfEncode {
  const uint64_t* fields;  // kMfFieldWords n; the comparator's {offset, length} are in names
  const uint8_t* names;
  uint64_t names_size;
  uint64_t n;
  const uint64_t* del_first;  // n + 1
  const uint64_t* del_items;
  uint64_t n_del;
  const uint64_t* new_first;  // n + 1
  const uint64_t* new_items;
  uint64_t n_new;
  const uint8_t* keys;
  const uint64_t* key_offsets;  // 2 n_new + 1
  uint64_t keys_size;
  uint64_t out_at;
  // the first call's outputs
  uint64_t* records;  // 2 n: {out_at + offset, length}
  uint64_t* totals;   // 1: bytes
  uint32_t* status;
  // the second call's outputs
  uint8_t* image;
  uint64_t out_cap;
  // scratch
  uint64_t* hdr;    // kMhWords
  uint64_t* pe;     // n + 1: the edits' sizes, summed
  uint64_t* pd;     // n_del + 1
  uint64_t* pn;     // n_new + 1
  uint64_t* tiles;  // one row of max tiles + 1
};

}  // namespace lsbm
