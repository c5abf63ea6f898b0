/*
 * lsbm_merge.h -- C ABI of the MI355X (gfx950) batched compaction merge: the
 * MergingIterator of lsbm's table/merger.cc over sorted runs and the drop rule
 * of DoCompactionWork, for all entries of a compaction in one launch sequence.
 * Implemented by lsbm_amd/liblsbm_crc32c.so with the conventions of
 * include/lsbm_block_build.h: extern "C", device pointers and an explicit
 * stream (`void*` hipStream_t), calls only enqueue, LSBM_* status codes, never
 * throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   table/merger.cc:155-168      MergingIterator::FindSmallest (the smallest
 *                                key; among equal keys the lowest child)
 *   common/dbformat.cc:50-66     InternalKeyComparator::Compare
 *   util/comparator.cc:25-27     BytewiseComparator::Compare
 *                                -> lsbm_merge_plan_dev
 *   lsbm/db_impl.cc:999-1032     DoCompactionWork's drop rule
 *                                -> lsbm_merge_plan_dev with LSBM_MERGE_DROP
 *   lsbm/db_impl.cc:1053         builder->Add(key, value) in merged order
 *                                -> lsbm_merge_gather_dev, whose output
 *                                lsbm_block_plan_dev / _build_dev read
 *
 * Entries are what lsbm_block_decode_dev writes:
 *   key e   = d_keys[d_key_offsets[e], d_key_offsets[e+1])   (keys_size bytes)
 *   value e = {d_values[2e], d_values[2e+1]} = {offset, length} in a value image
 * Run r owns entries [d_run_first[r], d_run_first[r+1]); the runs tile
 * [0, n_entries) and each is sorted under cmp (equal neighbours are legal).
 *
 * Order: LSBM_CMP_BYTEWISE is memcmp, then length; LSBM_CMP_INTERNAL_KEY is the
 * user key (all but the last 8 bytes) bytewise ascending, then the 64-bit
 * little-endian tag (seq << 8 | type) descending.  Among equal keys the
 * lowest-numbered run comes first, and inside a run the earlier entry: the
 * stable merge by (key, run, position).
 *
 * No byte outside the key buffer is read and no value byte at all; nothing is
 * written outside the outputs' stated sizes.  Outputs must not alias inputs:
 * where pointers and sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_MERGE_H_
#define LSBM_MERGE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_CMP_*, LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK ... LSBM_MERGE_UNSORTED */

#ifdef __cplusplus
extern "C" {
#endif

/* Per-run status of lsbm_merge_plan_dev, and d_status[0] of
 * lsbm_merge_gather_dev.  Several findings report the largest code.
 *   LSBM_MERGE_NO_ROOM    gather: out_keys_cap or entries_cap is smaller than
 *                         the output; nothing is written
 *   LSBM_MERGE_BAD_INPUT  key offsets decrease or pass keys_size; d_run_first
 *                         decreases, passes n_entries or does not tile
 *                         [0, n_entries); under LSBM_CMP_INTERNAL_KEY a key
 *                         shorter than 8 bytes.  gather: d_source and the
 *                         plan's offsets are not a plan of these entries
 *   LSBM_MERGE_UNSORTED   an adjacent pair of the run has
 *                         Compare(key[i], key[i+1]) > 0
 * LSBM_MERGE_OK 0, _NO_ROOM 1, _BAD_INPUT 2, _UNSORTED 3 are defined beside
 * the LSBM_BUILD_* codes in lsbm_block_build.h. */

#define LSBM_MERGE_MAX_RUNS 64u
/* the most entries one call takes (2^36) */
#define LSBM_MERGE_MAX_ENTRIES (1ull << 36)

/* flags of lsbm_merge_plan_dev */
#define LSBM_MERGE_DROP 0x1u         /* apply DoCompactionWork's drop rule (internal keys only) */
#define LSBM_MERGE_BOTTOM_LEVEL 0x2u /* the caller's statement that level() + 1 == kNumLevels */

/* Device scratch lsbm_merge_plan_dev needs (bytes; the caller allocates,
 * contents are the call's own). */
uint64_t lsbm_merge_scratch_bytes(uint64_t n_entries, uint64_t n_runs);

/* Which input entry becomes which output entry.
 *   d_source[j]           the input entry that becomes output entry j
 *                         (n_entries slots, d_counts[0] used)
 *   d_out_key_offsets[j]  where output key j starts in the output's key bytes
 *                         (n_entries + 1 slots, d_counts[0] + 1 used): the
 *                         running sum lsbm_merge_gather_dev copies by
 *   d_counts[0]           n_out, the entries of the output
 *   d_counts[1]           the key bytes of the output
 *   d_run_status[r]       LSBM_MERGE_* per run
 * If any run is in error n_out = 0 and d_source is unspecified.
 *
 * With flags & LSBM_MERGE_DROP (LSBM_ERR_INVALID unless cmp is
 * LSBM_CMP_INTERNAL_KEY) the entry at merged position p is left out when
 *   last_seq <= smallest_snapshot ||
 *   (type(p) == kTypeDeletion && seq(p) <= smallest_snapshot && (flags & LSBM_MERGE_BOTTOM_LEVEL))
 * where last_seq is seq(p - 1) if p - 1 exists, parses (its type byte is at
 * most kTypeValue) and has p's user key, and kMaxSequenceNumber (2^56 - 1)
 * otherwise.  An entry that does not parse is always kept. */
int lsbm_merge_plan_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                        uint64_t n_entries, const uint64_t* d_run_first, uint64_t n_runs, int cmp, uint32_t flags,
                        uint64_t smallest_snapshot, uint64_t* d_source, uint64_t* d_out_key_offsets,
                        uint64_t* d_counts, uint32_t* d_run_status, void* d_scratch, uint64_t scratch_bytes,
                        void* stream);

/* The output entries, in the shape of the input: key j at
 * d_out_keys[d_out_key_offsets[j], d_out_key_offsets[j+1]), value slice
 * d_out_values[2j], [2j+1] copied from the source entry (value bytes are not
 * moved: the slices still point into the input's value image).  n_out is read
 * from d_counts on the device, so no host read is needed between plan and
 * gather: out_keys_cap = keys_size and entries_cap = n_entries always suffice.
 *   d_plan_key_offsets  plan's d_out_key_offsets
 *   d_out_key_offsets   entries_cap + 1 slots
 *   d_out_values        2 x entries_cap slots
 *   d_status[0]         LSBM_MERGE_OK, _NO_ROOM or _BAD_INPUT */
int lsbm_merge_gather_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                          const uint64_t* d_values, uint64_t n_entries, const uint64_t* d_source,
                          const uint64_t* d_plan_key_offsets, const uint64_t* d_counts, uint8_t* d_out_keys,
                          uint64_t out_keys_cap, uint64_t* d_out_key_offsets, uint64_t* d_out_values,
                          uint64_t entries_cap, uint32_t* d_status, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_MERGE_H_ */
