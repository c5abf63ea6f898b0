/*
 * lsbm_range.h -- C ABI of the MI355X (gfx950) range query of LSbM's buffered
 * tree: which files each query reads, in which order, and how many entries of
 * each it counts.  Implemented by lsbm_amd/liblsbm_crc32c.so with the
 * conventions of include/lsbm_probe.h: extern "C", device pointers and an
 * explicit stream (`void*` hipStream_t), calls only enqueue, LSBM_* status
 * codes, never throws.
 *
 * Reference interface replaced (lsbm = tengdj/lsbm):
 *   lsbm/version_set.cc:1043-1214  Version::RangeQuery's walk over
 *                                  levels_[level][type] under checkwb,
 *                                  wb_covered, dl_covered and cb_covered
 *                                              -> lsbm_range_plan_dev,
 *                                                 lsbm_range_emit_dev
 *   common/table_cache.cc:87-104   TableCache::GetRange
 *   table/table.cc:340-368         Table::InternalGetRange: Seek, then count
 *                                  up to the end key
 *                                              -> lsbm_range_count_dev
 *
 * A *slot* is one sorted table the walk can reach, in the fixed order in which
 * Version::RangeQuery can reach it: Level 0's head deletion table (ALL: every
 * file is tested, in the list's order) and its head insertion table (L0INS),
 * then per level 1..3 the warm-up tables from the list's head round (WB), the
 * head deletion table (DEL), the compaction-buffer tables from
 * levels_[L][2]->next round (CB) and the head insertion table (INS).  Slot s
 * holds the run entries [d_run_first[s], d_run_first[s + 1]) (n_slots + 1
 * numbers, the first 0 and the last n_runs); run entry r has the smallest and
 * largest internal keys of its file at d_bounds[d_bound_offsets[2r] ..
 * d_bound_offsets[2r + 1]) and [.. d_bound_offsets[2r + 2]) (2 n_runs + 1
 * offsets), 8 bytes at least each.
 *
 * d_slot_info[s] = kind | level << 8 | flags << 16.  The slots are sorted by
 * (level, kind); only WB and CB repeat in a level; level-0 slots have the kinds
 * ALL and L0INS and no other level does.  LSBM_RANGE_COVERS marks the WB or CB
 * table whose ->next is the walk head's ->prev in the full circular list;
 * LSBM_RANGE_SOLE marks a CB table that is its list's only one.
 *
 * Per query (start and end are the user keys of its two lookup keys) a file
 * *overlaps* when end >= its smallest user key and start <= its largest.  A
 * *walk* of a slot begins at FindFile(icmp, files, start) -- the binary search
 * of lsbm/version_set.cc:130-150 handed the user key, whose last 8 bytes the
 * internal comparator reads as a tag -- pushes every overlapping file from
 * there on and stops after the first file with end < its smallest user key.  An
 * ALL slot pushes every overlapping file and never stops early.
 *
 *   Level 0: ALL, then the walk of L0INS.
 *   Level L = 1..3 (u = d_use_len[L], w = d_use_len[L - 1]):
 *     checkwb = d_wb_enabled[L] != 0 && start > cursor key L
 *     if checkwb: the walks of the WB slots j = 0.. with j <= w; wb_covered if
 *       a COVERS slot pushed a file
 *     if wb_covered: those files are read; else they are dropped and DEL is
 *       walked, dl_covered if it pushed a file
 *     if u > 0 && end < cursor key 4 (read_upto_key): the walks of the CB slots
 *       j = 0.. with j < u; after wb_covered || dl_covered slot 0 is left out,
 *       but a SOLE slot 0 is walked if u >= 2; cb_covered if a COVERS slot
 *       pushed a file
 *     if cb_covered: those files are read; else they are dropped and INS is
 *       walked
 *   The files of level 0 are read with level 1's.  A pair's flag word is
 *   LSBM_RANGE_LAST (the last file read for its level: levels 0 and 1 are one
 *   group) | the slot's level << 8.  d_checked[q] is the number of files read.
 *   d_wb_enabled[L] is the caller's `buffered_merge && L > 1 && use_len[L-1] > 0`.
 *
 * The two-call pattern of the library: lsbm_range_plan_dev writes d_count[q];
 * the caller's exclusive prefix sum is d_pair_first (n_queries + 1 numbers);
 * lsbm_range_emit_dev writes pair d_pair_first[q] + j, j < count[q].
 *
 * lsbm_range_count_dev reads the *range index*: the internal keys of every
 * entry of every file, file after file in table order, entry e at
 * d_index_keys[d_index_offsets[e], d_index_offsets[e + 1]); file f holds the
 * entries [d_file_first_entry[f], d_file_first_entry[f + 1]); a file with
 * d_file_state[f] != 0 did not open for iteration and has no entries.  Per pair
 * it finds the lower bound of the start lookup key under the internal
 * comparator (the two-level iterator's Seek) and counts from there to the
 * first entry whose whole internal key is bytewise greater than the whole end
 * lookup key, or to the file's end.  That predicate is not monotone in the
 * table's order (the tags compare as little-endian bytes; a longer user key may
 * sort below the end key's tag), so the first entry that meets it is found by
 * stepping, not by a search.
 *
 * Every call has one status word, d_status[0]: LSBM_MERGE_OK; or
 * LSBM_MERGE_BAD_INPUT where a slot's level is above 3, its kind or a flag
 * unknown, the slots are not sorted, d_run_first or an offset list decreases
 * or passes its buffer, a bound is under 8 bytes, a start or end lookup key is
 * under 16 bytes, (emit) d_pair_first does not step by the counts, (count)
 * d_pair_first decreases or does not end at n_pairs, a pair names a file that
 * is not there, or an index key is under 8 bytes; or (emit)
 * LSBM_MERGE_NO_ROOM where d_pair_first[n_queries] > pair_cap.  On either
 * nothing is written but the status word.  No byte outside a stated size is
 * read or written.  Outputs must not alias inputs: where pointers and sizes
 * show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_RANGE_H_
#define LSBM_RANGE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_RANGE_LEVELS 4u /* config::kNumLevels: the entries of d_use_len and d_wb_enabled */
#define LSBM_RANGE_CURSORS 5u /* read_cursor_key_[0..3], then read_upto_key_ */

/* slot kinds, in the order of a level's slots */
#define LSBM_RANGE_SLOT_ALL 0u
#define LSBM_RANGE_SLOT_L0INS 1u
#define LSBM_RANGE_SLOT_WB 2u
#define LSBM_RANGE_SLOT_DEL 3u
#define LSBM_RANGE_SLOT_CB 4u
#define LSBM_RANGE_SLOT_INS 5u

/* slot flags (d_slot_info >> 16) */
#define LSBM_RANGE_COVERS 1u
#define LSBM_RANGE_SOLE 2u

/* pair flags */
#define LSBM_RANGE_LAST 1u
#define LSBM_RANGE_NO_ENTRIES 2u /* set by the caller from d_pair_error */

/* d_count[q] = the number of files query q reads.  The lookup keys are those
 * of lsbm_lookup_keys_dev (user key || 8-byte tag); cursor key i is
 * d_cursor_keys[d_cursor_offsets[i], d_cursor_offsets[i + 1]) (LSBM_RANGE_CURSORS
 * + 1 offsets), a user key.  One lane per query. */
int lsbm_range_plan_dev(const uint32_t* d_slot_info, uint64_t n_slots, const uint64_t* d_run_first, uint64_t n_runs,
                        const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets,
                        const uint32_t* d_use_len, const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys,
                        uint64_t cursor_keys_size, const uint64_t* d_cursor_offsets, const uint8_t* d_start_keys,
                        uint64_t start_keys_size, const uint64_t* d_start_offsets, const uint8_t* d_end_keys,
                        uint64_t end_keys_size, const uint64_t* d_end_offsets, uint64_t n_queries, uint32_t* d_count,
                        uint32_t* d_status, void* stream);

/* Pair p = d_pair_first[q] + j is the j-th file query q reads, in the
 * reference's order: d_pair_run[p] its run entry, d_pair_flags[p] its flag
 * word; d_checked[q] = count[q].  The inputs are those of the plan call,
 * unchanged. */
int lsbm_range_emit_dev(const uint32_t* d_slot_info, uint64_t n_slots, const uint64_t* d_run_first, uint64_t n_runs,
                        const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets,
                        const uint32_t* d_use_len, const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys,
                        uint64_t cursor_keys_size, const uint64_t* d_cursor_offsets, const uint8_t* d_start_keys,
                        uint64_t start_keys_size, const uint64_t* d_start_offsets, const uint8_t* d_end_keys,
                        uint64_t end_keys_size, const uint64_t* d_end_offsets, uint64_t n_queries,
                        const uint64_t* d_pair_first, uint32_t* d_pair_run, uint32_t* d_pair_flags, uint64_t pair_cap,
                        uint32_t* d_checked, uint32_t* d_status, void* stream);

/* d_pair_count[p] = TableCache::GetRange of pair p's file (d_pair_file[p], an
 * index into the range index's files) for its query; d_pair_error[p] = 1 where
 * the file has no entries to iterate (d_file_state), else 0.  d_found[q] = the
 * sum of the counts of q's pairs flagged LSBM_RANGE_LAST (Version::RangeQuery's
 * return value); d_total[q] = the sum of all of q's counts (no reference
 * figure).  One wave per pair, then one lane per query. */
int lsbm_range_count_dev(const uint8_t* d_index_keys, uint64_t index_keys_size, const uint64_t* d_index_offsets,
                         uint64_t n_entries, const uint64_t* d_file_first_entry, const uint32_t* d_file_state,
                         uint64_t n_files, const uint8_t* d_start_keys, uint64_t start_keys_size,
                         const uint64_t* d_start_offsets, const uint8_t* d_end_keys, uint64_t end_keys_size,
                         const uint64_t* d_end_offsets, uint64_t n_queries, const uint64_t* d_pair_first,
                         const uint32_t* d_pair_file, const uint32_t* d_pair_flags, uint64_t n_pairs,
                         uint32_t* d_pair_count, uint32_t* d_pair_error, uint32_t* d_found, uint64_t* d_total,
                         uint32_t* d_status, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_RANGE_H_ */
