// include/lsbm/compaction.h -- C++ host API for the middle of lsbm's
// DoCompactionWork (lsbm/db_impl.cc): the merge of the input tables' entries
// and the cut of the merged entries into output files, over host buffers.
//
// Mirrors, for all entries of a compaction at once, what the reference does
// per key:
//   MergingIterator over the inputs (table/merger.cc:155-168) and the drop
//   rule (lsbm/db_impl.cc:999-1032)                    -> MergeRuns
//   "close the output file once FileSize() >= MaxOutputFileSize()"
//   (lsbm/db_impl.cc:1056-1064)                        -> CutTables
// MergeRuns sits on top of the C ABI (include/lsbm_merge.h); the entries are
// merged on the GPU.  CutTables is host arithmetic over a plan's block sizes.
// Entries are what DecodeBlocks (include/lsbm/block_reader.h) returns and what
// PlanBlocks / BuildBlocks (include/lsbm/block_builder.h) read.  No HIP types
// in this header.
#ifndef LSBM_COMPACTION_H_
#define LSBM_COMPACTION_H_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "lsbm/block_builder.h"  // BlockEntries
#include "lsbm/block_reader.h"   // BlockComparator
#include "lsbm/status.h"

namespace lsbm {

struct MergeOptions {
  BlockComparator cmp = kInternalKeyComparator;
  bool drop = false;                 // apply DoCompactionWork's drop rule (internal keys only)
  uint64_t smallest_snapshot = 0;    // compact->smallest_snapshot
  bool bottom_level = false;         // level() + 1 == kNumLevels
};

// Run r owns entries [run_first[r], run_first[r+1]) of `entries`, sorted under
// opt.cmp; at most 64 runs.  The merged (and, with opt.drop, thinned) entries:
// output entry j is input entry (*source)[j], its key
// (*keys)[(*key_offsets)[j], (*key_offsets)[j+1]) and its value slice
// (*values)[2j], [2j+1], still pointing into entries.value_image.
// (*run_statuses)[r]: LSBM_MERGE_*.  Returns InvalidArgument naming the first
// run in error; the outputs are then empty.
Status MergeRuns(int device, const BlockEntries& entries, const uint64_t* run_first, size_t n_runs,
                 const MergeOptions& opt, std::string* keys, std::vector<uint64_t>* key_offsets,
                 std::vector<uint64_t>* values, std::vector<uint64_t>* source, std::vector<uint32_t>* run_statuses);

// Where DoCompactionWork closes its output files.  block_first / block_bytes
// are the single-table plan of the merged entries (PlanBlocks with one table):
// TableBuilder::FileSize() grows only when a block is flushed, by the block and
// its 5-byte trailer, so table t ends after the first block at which the sum of
// block_bytes + 5 since its start reaches max_file_size, and the last block
// closes the last table.  Table t owns entries [(*table_first)[t],
// (*table_first)[t+1]) and blocks [(*table_block_first)[t],
// (*table_block_first)[t+1]); without blocks there are no tables.
Status CutTables(const uint64_t* block_first, const uint64_t* block_bytes, size_t n_blocks, uint64_t max_file_size,
                 std::vector<uint64_t>* table_first, std::vector<uint64_t>* table_block_first);

}  // namespace lsbm

#endif  // LSBM_COMPACTION_H_
