/*
 * lsbm_get.h -- C ABI of the MI355X (gfx950) batched DB::Get: the lookup key,
 * the memtable lookup, the file pick and the callback that decides, for many
 * queries in one launch each.  Implemented by lsbm_amd/liblsbm_crc32c.so with
 * the conventions of include/lsbm_merge.h and include/lsbm_memtable.h:
 * extern "C", device pointers and an explicit stream (`void*` hipStream_t),
 * calls only enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   common/dbformat.cc:121-137     LookupKey            -> lsbm_lookup_keys_dev
 *   common/memtable.cc:109-144     MemTable::Get        -> lsbm_memtable_get_dev
 *   lsbm/version_set.cc:130-150    FindFile, the smallest-key test beside it
 *   lsbm/version_set.cc:364-374    Level 0's overlap rule
 *                                                       -> lsbm_find_file_dev
 *   lsbm/version_set.cc:227-240    SaveValue
 *   lsbm/version_set.cc:392-407    `if (!s.ok()) return s` and the switch
 *                                                       -> lsbm_save_value_dev
 *
 * Keys are a uint8 buffer plus uint64 offsets (key i = keys[off[i], off[i+1])),
 * as everywhere else in the library.  The table reads between the file pick
 * and the callback are lsbm_block_seek_dev, lsbm_filter_block_may_match_dev
 * and the block reader of lsbm_amd/sstable.py; lsbm_amd/db.py is the chain.
 *
 * A per-query verdict word threads through the probe calls.  A call never
 * touches a query whose verdict is decided on entry: the first decisive source
 * wins and an error stops the search, as in Version::Get.  d_where[q] receives
 * the id of the source that decided.
 *
 * Every call has one status word, d_status[0]: LSBM_MERGE_OK, or
 * LSBM_MERGE_BAD_INPUT where an offsets array decreases, passes its buffer's
 * size or names a key shorter than the call needs.  On LSBM_MERGE_BAD_INPUT no
 * verdict, value or where word changes and no key byte is read.  No byte
 * outside a stated size is read or written.  Outputs must not alias inputs:
 * where pointers and sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_GET_H_
#define LSBM_GET_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes, LSBM_SEEK_* */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

/* per-query verdict */
#define LSBM_GET_UNDECIDED 0u /* keep searching (kNotFound) */
#define LSBM_GET_FOUND 1u     /* kFound */
#define LSBM_GET_DELETED 2u   /* kDeleted: NotFound, decisive */
#define LSBM_GET_CORRUPT 3u   /* kCorrupt: Corruption("corrupted key for ", user_key) */
#define LSBM_GET_ERROR 16u    /* + s: a table read's non-OK state s, `if (!s.ok()) return s` */

/* table-read states lsbm_save_value_dev takes: LSBM_SEEK_* and, from the chain
 * of lsbm_amd/sstable.py, */
#define LSBM_GET_STATE_FILTERED 6u       /* the filter says no: a miss */
#define LSBM_GET_STATE_BAD_CHECKSUM 7u   /* Corruption("block checksum mismatch") */
#define LSBM_GET_STATE_BAD_TYPE 8u       /* Corruption("bad block type") */
#define LSBM_GET_STATE_BAD_COMPRESSED 9u /* Corruption("corrupted compressed block contents") */
#define LSBM_GET_STATE_MAX 15u

/* run flags of lsbm_find_file_dev */
#define LSBM_RUN_LEVEL0 0x1u     /* one file that may overlap its neighbours: the user-key range test */
#define LSBM_RUN_PRECHECKED 0x2u /* ContainKey, then SkipFilterGet (the chain's business; the pick ignores it) */

/* LookupKey for n_queries user keys: key q of the output is
 *   user key q || fixed64(seq << 8 | 1)      (kValueTypeForSeek = kTypeValue)
 * with seq = d_snapshots[q], or `snapshot` when d_snapshots is NULL, and
 *   d_key_offsets[q] = d_user_offsets[q] + 8q     (n_queries + 1 slots).
 * LSBM_MERGE_BAD_INPUT: user offsets that decrease or pass user_keys_size, or
 * keys_cap < d_user_offsets[n_queries] + 8 n_queries; nothing is written then. */
int lsbm_lookup_keys_dev(const uint8_t* d_user_keys, uint64_t user_keys_size, const uint64_t* d_user_offsets,
                         uint64_t n_queries, uint64_t snapshot, const uint64_t* d_snapshots, uint8_t* d_keys,
                         uint64_t keys_cap, uint64_t* d_key_offsets, uint32_t* d_status, void* stream);

/* MemTable::Get over a sorted memtable: n_entries internal keys in the order
 * of lsbm_memtable_sort_dev (user key ascending, tag descending) with their
 * {offset, length} value slices, as lsbm_merge_gather_dev leaves them.  Per
 * undecided query: the first entry >= the lookup key; if there is one and its
 * user key equals the query's, the tag's low byte decides -- kTypeValue:
 * LSBM_GET_FOUND and d_value[2q], [2q+1] = the entry's slice; kTypeDeletion:
 * LSBM_GET_DELETED and {0, 0}; d_where[q] = source_id.  Any other case leaves
 * the query as it is.  One lane per query.
 * LSBM_MERGE_BAD_INPUT: a memtable key or a lookup key under 8 bytes, offsets
 * that decrease or pass their buffer's size (mem_check's rule). */
int lsbm_memtable_get_dev(const uint8_t* d_mem_keys, uint64_t mem_keys_size, const uint64_t* d_mem_key_offsets,
                          const uint64_t* d_mem_values, uint64_t n_entries, const uint8_t* d_keys, uint64_t keys_size,
                          const uint64_t* d_key_offsets, uint64_t n_queries, int32_t source_id, uint32_t* d_verdict,
                          uint64_t* d_value, int32_t* d_where, uint32_t* d_status, void* stream);

/* The file each run offers each query.  File f's bounds are the internal keys
 * 2f (smallest) and 2f + 1 (largest) of d_bounds / d_bound_offsets
 * (2 n_files + 1 slots); run r holds files [d_run_first[r], d_run_first[r+1]),
 * in key order.  One lane per (query, run):
 *   a sorted run: FindFile's binary search, the least i with
 *     icmp(largest_i, lookup key) >= 0; then user_key >= smallest_i.user_key();
 *     then d_visible[i] != 0;
 *   a run flagged LSBM_RUN_LEVEL0 holds at most one file, a candidate iff
 *     smallest.user_key() <= user_key <= largest.user_key() (sequences are not
 *     compared, and d_visible is not read: version_set.cc:364-374).
 * d_file[q * n_runs + r] = the file's index, or -1.
 * LSBM_MERGE_BAD_INPUT (every d_file word written is -1): a bound or a lookup
 * key under 8 bytes, offsets that decrease or pass their buffer's size, a
 * d_run_first that decreases or passes n_files, a LEVEL0 run of two files or
 * more. */
int lsbm_find_file_dev(const uint8_t* d_bounds, uint64_t bounds_size, const uint64_t* d_bound_offsets,
                       uint64_t n_files, const uint64_t* d_run_first, const uint32_t* d_run_flags,
                       const uint8_t* d_visible, uint64_t n_runs, const uint8_t* d_keys, uint64_t keys_size,
                       const uint64_t* d_key_offsets, uint64_t n_queries, int32_t* d_file, uint32_t* d_status,
                       void* stream);

/* SaveValue and the switch after it over one round's table reads.  Per
 * undecided query, d_state[q] is the read's state:
 *   LSBM_SEEK_NOT_VALID, LSBM_GET_STATE_FILTERED   nothing changes
 *   any other state but LSBM_SEEK_VALID            LSBM_GET_ERROR + state
 *   LSBM_SEEK_VALID: the found key has d_key_len[q] bytes, of which the window
 *     d_found[d_found_offsets[q], d_found_offsets[q+1]) holds the first ones
 *     (lsbm_block_seek_dev's), and the value slice d_value_in[2q], [2q+1].
 *     ParseInternalKey first: a length under 8 or a type byte above 1 gives
 *     LSBM_GET_CORRUPT.  Otherwise an equal user key gives LSBM_GET_FOUND with
 *     d_value[2q], [2q+1] = the slice, or LSBM_GET_DELETED with {0, 0}; another
 *     user key changes nothing.
 * d_value and d_where[q] = source_id are written only for queries the call
 * decides.
 * LSBM_MERGE_BAD_INPUT: a state above LSBM_GET_STATE_MAX, a lookup key under
 * 8 bytes, offsets that decrease or pass their buffer's size, or an undecided
 * valid query whose key of 8 bytes or more does not fit its window. */
int lsbm_save_value_dev(const uint32_t* d_state, const uint64_t* d_key_len, const uint8_t* d_found,
                        uint64_t found_size, const uint64_t* d_found_offsets, const uint64_t* d_value_in,
                        const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_queries,
                        int32_t source_id, uint32_t* d_verdict, uint64_t* d_value, int32_t* d_where,
                        uint32_t* d_status, void* stream);

/* The values themselves: for every query with where_lo <= d_where[q] <
 * where_hi, image[d_slices[2q], + d_slices[2q+1]) is copied to
 * d_out[d_out_offsets[q], ...) (n_queries + 1 slots).  Other queries' bytes
 * are not written.
 * LSBM_MERGE_BAD_INPUT: a selected slice that is not inside the image, or that
 * is longer than d_out_offsets[q+1] - d_out_offsets[q], or a window that is
 * not inside out_cap; such a query is not copied, the others are. */
int lsbm_slices_gather_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_slices,
                           const int32_t* d_where, int32_t where_lo, int32_t where_hi, uint8_t* d_out,
                           uint64_t out_cap, const uint64_t* d_out_offsets, uint64_t n_queries, uint32_t* d_status,
                           void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_GET_H_ */
