/*
 * lsbm_iter.h -- C ABI of the MI355X (gfx950) batched range scan: the DBIter of
 * lsbm's lsbm/db_iter.cc (NewIterator / Seek / SeekToFirst / SeekToLast / Next /
 * Prev / status) over merged entries at a snapshot, for many range queries in
 * one launch sequence.  Implemented by lsbm_amd/liblsbm_crc32c.so with the
 * conventions of include/lsbm_merge.h and include/lsbm_get.h: extern "C",
 * device pointers and an explicit stream (`void*` hipStream_t), calls only
 * enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   lsbm/db_iter.cc:172-202   FindNextUserEntry  -> lsbm_dbiter_plan_dev
 *   lsbm/db_iter.cc:231-271   FindPrevUserEntry  (the same set of entries)
 *   lsbm/db_iter.cc:273-303   Seek, SeekToFirst, SeekToLast
 *   lsbm/db_iter.cc:145-170   Next               -> lsbm_dbiter_range_dev
 *   lsbm/db_iter.cc:204-229   Prev
 *   lsbm/db_iter.cc:74-80     status()
 *   key() / value()                              -> lsbm_dbiter_emit_dev
 * The internal iterator under DBIter (lsbm/db_impl.cc:1139-1157, a
 * MergingIterator over memtables and tables) is lsbm_merge_plan_dev /
 * lsbm_merge_gather_dev without the drop rule.
 *
 * Two stages.  A snapshot view is built once per (entries, snapshot) and holds
 * the user-visible sequence; scans then answer range queries against it with
 * binary searches and copies.
 *
 * Entries are n internal keys sorted under InternalKeyComparator, in the shape
 * lsbm_block_decode_dev / lsbm_merge_gather_dev write:
 *   key p = d_keys[d_key_offsets[p], d_key_offsets[p+1])   (keys_size bytes)
 * With s the snapshot, for merged position p:
 *   parses(p)     the type byte is at most kTypeValue (1)
 *   visible(p)    parses(p) && seq(p) <= s
 *   corrupt(p)    !parses(p)
 *   seg_start(p)  p == 0, or the user key differs from p-1's
 *   head(p)       visible(p), and no visible p' < p has p's user key
 *   yield(p)      head(p) && type(p) == kTypeValue
 * The yielded entries, ascending, are what a DBIter at s steps over in either
 * direction; a corrupt entry is stepped over and sets status().
 *
 * Each call has one status word, LSBM_MERGE_OK (0), _NO_ROOM (1), _BAD_INPUT (2)
 * or _UNSORTED (3) (include/lsbm_block_build.h).  On an error found by a call's
 * check kernels nothing but that word is written.  No byte is read outside the
 * checked offsets; plan and range read no value byte.  Outputs must not alias
 * inputs or each other: where pointers and sizes show an overlap the call
 * returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_ITER_H_
#define LSBM_ITER_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK ... LSBM_MERGE_UNSORTED */

#ifdef __cplusplus
extern "C" {
#endif

/* per-query status of a scan: Status::ToString() is "OK" or
 * "Corruption: corrupted internal key in DBIter" */
#define LSBM_SCAN_OK 0u
#define LSBM_SCAN_CORRUPTION 1u

/* the most entries one view takes (2^36), and the most queries one call takes */
#define LSBM_DBITER_MAX_ENTRIES (1ull << 36)
#define LSBM_DBITER_MAX_QUERIES (1ull << 31)

/* Device scratch lsbm_dbiter_plan_dev needs (bytes; the caller allocates,
 * 8-byte aligned, contents are the call's own). */
uint64_t lsbm_dbiter_scratch_bytes(uint64_t n_entries);

/* The snapshot view of n_entries sorted entries at `snapshot`.
 *   d_source[j]           live[j]: the merged position of the j-th yielded
 *                         entry (n_entries slots, d_counts[0] used)
 *   d_out_key_offsets[j]  where live entry j's internal key starts among the
 *                         live keys (n_entries + 1 slots, d_counts[0] + 1 used)
 *   d_counts[0]           n_yield
 *   d_counts[1]           the key bytes of the live entries
 *   d_counts[2]           the corrupt entries
 * d_source, d_out_key_offsets and d_counts[0..1] are exactly what
 * lsbm_merge_plan_dev writes, so lsbm_merge_gather_dev materialises the live
 * entries (internal keys and value slices) from them unchanged.
 *   d_yield_rank[p]       yields before position p     (n_entries + 1 slots)
 *   d_corrupt_rank[p]     corrupt entries before p     (n_entries + 1 slots)
 *   d_first[j]            the seg_start position of live[j]'s user key
 *   d_back[j]             the largest visible position below d_first[j], or -1
 *                         (n_entries slots each, d_counts[0] used)
 *   d_status[0]           LSBM_MERGE_OK; _BAD_INPUT: key offsets decrease or
 *                         pass keys_size, or a key is shorter than 8 bytes;
 *                         _UNSORTED: an adjacent pair has Compare > 0.  Then
 *                         nothing else is written: a caller that chains the
 *                         gather without reading the word zeroes d_counts first.
 * Equal neighbours are legal (the same internal key in two children). */
int lsbm_dbiter_plan_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                         uint64_t n_entries, uint64_t snapshot, uint64_t* d_source, uint64_t* d_out_key_offsets,
                         uint64_t* d_counts, uint64_t* d_yield_rank, uint64_t* d_corrupt_rank, uint64_t* d_first,
                         int64_t* d_back, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* A batch of range queries against a view, one fresh iterator each: the
 * half-open user-key interval [lo, hi), at most `limit` entries, forward
 *   Seek(lo) or SeekToFirst(); while (Valid() && key() < hi) Next()
 * or, with `reverse`, the same interval from its end
 *   Seek(hi), then Prev() if Valid() else SeekToLast(); or SeekToLast();
 *   while (Valid() && key() >= lo) Prev()
 * both stopped after `limit` entries without a further Next() / Prev();
 * limit 0 makes no call at all.
 *   d_keys ... n_entries, snapshot   the entries and snapshot the view was planned from
 *   d_live, d_live_key_offsets, d_counts, d_yield_rank, d_corrupt_rank,
 *   d_first, d_back                  the plan's outputs
 *   d_value_prefix[j]                the value bytes of live entries before j
 *                                    (n_yield + 1 slots)
 *   d_lo_keys / d_lo_offsets         query q's lo is bytes [off[q], off[q+1]);
 *   d_lo_present[q]                  0: no lower bound (SeekToFirst).  A null
 *                                    d_lo_present means every query has one
 *   d_hi_keys / d_hi_offsets / d_hi_present   the same for hi; a null
 *                                    d_hi_offsets means no query has one
 *   d_limits                         one limit per query, or null: `limit`
 * Writes, per query,
 *   d_j_begin[q], d_count[q]  the window live[j_begin, j_begin + count), which
 *                             a reverse scan returns last entry first
 *   d_scan_status[q]          LSBM_SCAN_OK or LSBM_SCAN_CORRUPTION: whether
 *                             ParseKey ran on a corrupt entry during the calls
 *                             above (DESIGN.md section 18 lists the positions)
 *   d_key_bytes[q], d_value_bytes[q]   the user-key and value bytes of the window
 *   d_status[0]               LSBM_MERGE_OK; _BAD_INPUT: entry or query offsets
 *                             decrease or pass their buffer, a key shorter than
 *                             8 bytes (then nothing else is written), or the
 *                             view is not a plan of these entries (then the
 *                             per-query outputs are unspecified). */
int lsbm_dbiter_range_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                          uint64_t n_entries, uint64_t snapshot, const uint64_t* d_live,
                          const uint64_t* d_live_key_offsets, const uint64_t* d_counts, const uint64_t* d_yield_rank,
                          const uint64_t* d_corrupt_rank, const uint64_t* d_first, const int64_t* d_back,
                          const uint64_t* d_value_prefix, const uint8_t* d_lo_keys, uint64_t lo_keys_size,
                          const uint64_t* d_lo_offsets, const uint8_t* d_lo_present, const uint8_t* d_hi_keys,
                          uint64_t hi_keys_size, const uint64_t* d_hi_offsets, const uint8_t* d_hi_present,
                          uint64_t n_queries, uint64_t limit, const uint64_t* d_limits, int reverse,
                          uint64_t* d_j_begin, uint64_t* d_count, uint32_t* d_scan_status, uint64_t* d_key_bytes,
                          uint64_t* d_value_bytes, uint32_t* d_status, void* stream);

/* The entries of every query's window, query after query.
 *   d_j_begin                     from lsbm_dbiter_range_dev
 *   d_entry_first, d_key_first, d_value_first
 *                                 the exclusive sums of d_count, d_key_bytes and
 *                                 d_value_bytes (n_queries + 1 slots each)
 *   d_live_keys, d_live_key_offsets, d_live_values, n_live
 *                                 the live entries as lsbm_merge_gather_dev
 *                                 wrote them from the plan
 *   d_value_prefix                as above
 *   d_image                       the value image the slices point into
 * Output entry i of query q is number i - d_entry_first[q] of its window,
 * ascending, or descending with `reverse`:
 *   d_out_keys[d_out_key_offsets[i], d_out_key_offsets[i+1])        its user key
 *   d_out_values[d_out_value_offsets[i], d_out_value_offsets[i+1])  its value
 * (entries_cap + 1 offset slots each).
 *   d_status[0]  LSBM_MERGE_OK; _NO_ROOM: entries_cap, out_keys_cap or
 *                out_values_cap is smaller than the sums' ends, nothing is
 *                written; _BAD_INPUT: a prefix array decreases (nothing is
 *                written), or the windows, the live entries and the sums do
 *                not belong together (no byte of such a wave is moved). */
int lsbm_dbiter_emit_dev(const uint64_t* d_j_begin, const uint64_t* d_entry_first, const uint64_t* d_key_first,
                         const uint64_t* d_value_first, uint64_t n_queries, int reverse, const uint8_t* d_live_keys,
                         uint64_t live_keys_size, const uint64_t* d_live_key_offsets, const uint64_t* d_live_values,
                         uint64_t n_live, const uint64_t* d_value_prefix, const uint8_t* d_image, uint64_t image_size,
                         uint8_t* d_out_keys, uint64_t out_keys_cap, uint64_t* d_out_key_offsets,
                         uint8_t* d_out_values, uint64_t out_values_cap, uint64_t* d_out_value_offsets,
                         uint64_t entries_cap, uint32_t* d_status, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_ITER_H_ */
