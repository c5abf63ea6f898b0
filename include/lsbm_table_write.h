/*
 * lsbm_table_write.h -- C ABI of the MI355X (gfx950) batched table finish: what
 * TableBuilder::Finish does between the data blocks and the footer, for many
 * tables in one chain, and the sort that keeps the memtables of one log apart.
 * Implemented by lsbm_amd/liblsbm_crc32c.so with the conventions of
 * include/lsbm_merge.h: extern "C", device pointers and an explicit stream
 * (`void*` hipStream_t), calls only enqueue, the library allocates nothing on
 * the device, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   table/table_builder.cc:176-255  WriteBlock / WriteRawBlock for every table
 *                                   of a batch -> lsbm_table_pack_plan_dev
 *   table/filter_block.cc:22-76     FilterBlockBuilder::StartBlock, AddKey,
 *                                   Finish, GenerateFilter's bookkeeping
 *                                   -> lsbm_filter_layout_dev
 *   table/table_builder.cc:213-232  Finish: the metaindex block's one entry
 *                                   -> lsbm_metaindex_build_dev
 *   table/format.cc:32-42           Footer::EncodeTo -> lsbm_table_place_dev
 *   common/skiplist.h:334-367       the skiplist's order, one list per memtable
 *                                   -> lsbm_memtable_sort_segments_dev
 *
 * Tables.  Table t owns the data blocks [table_block_first[t],
 * table_block_first[t + 1]) of a batch of n_blocks blocks and the entries
 * [block_first[table_block_first[t]], block_first[table_block_first[t + 1]]).
 * table_block_first has n_tables + 1 words, begins with 0, never decreases and
 * ends with n_blocks; one that does not makes every table of the call
 * LSBM_BUILD_BAD_INPUT and the call writes nothing else.  Handles are {offset,
 * size} pairs of uint64 and relative to their table's first byte until
 * lsbm_table_place_dev adds the table's base.
 *
 * Per-table status words are LSBM_BUILD_OK, LSBM_BUILD_NO_ROOM and
 * LSBM_BUILD_BAD_INPUT (include/lsbm_block_build.h).  A table in error stores
 * nothing in its windows and does not affect the others.  No byte outside the
 * stated windows is read or written.  Outputs must not alias inputs: where
 * pointers and sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_TABLE_WRITE_H_
#define LSBM_TABLE_WRITE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block_build.h" /* LSBM_BUILD_*, LSBM_MERGE_*, LSBM_* status codes */
#include "lsbm_memtable.h"    /* LSBM_MEMTABLE_MAX_ENTRIES */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_TABLE_WRITE_MAX_BLOCKS (1ull << 31)
#define LSBM_TABLE_WRITE_MAX_TABLES (1ull << 31)
#define LSBM_TABLE_FOOTER_BYTES 48ull        /* table/format.h:70 */
#define LSBM_TABLE_NO_PLACE UINT64_MAX       /* filter_out of a filter whose table is in error */

/* Device scratch of the three calls below that take one (bytes; the caller
 * allocates, 8-byte aligned; contents are the call's own). */
uint64_t lsbm_table_write_scratch_bytes(uint64_t n_blocks, uint64_t n_tables);

/* lsbm_block_pack_plan_dev's rule with the running offset restarting at every
 * table: per block of table t
 *   type[i]   = d_comp_len[i] != UINT64_MAX
 *               && d_comp_len[i] < d_raw_len[i] - d_raw_len[i] / 8   ? 1 : 0
 *   size[i]   = type[i] ? d_comp_len[i] : d_raw_len[i]
 *   offset[i] = first_offset[t] + sum over the table's blocks j < i of (size[j] + gap)
 *   d_end[t]  = the offset after the table's last block's gap (first_offset[t]
 *               for a table without blocks)
 * d_comp_len == NULL: every block stays raw.  d_first_offset == NULL: 0 for
 * every table.  Sums wrap at 2^64.  The same call lays out the data blocks
 * (first_offset NULL) and the two or three blocks that follow them in every
 * table (first_offset = the data blocks' d_end; the filter block's comp_len is
 * UINT64_MAX, as WriteRawBlock(kNoCompression) writes it raw).
 * Outputs: d_types[n_blocks], d_handles[2 n_blocks], d_end[n_tables],
 * d_status[n_tables]. */
int lsbm_table_pack_plan_dev(const uint64_t* d_raw_len, const uint64_t* d_comp_len, uint64_t n_blocks,
                             const uint64_t* d_table_block_first, uint64_t n_tables, const uint64_t* d_first_offset,
                             uint64_t gap, uint8_t* d_types, uint64_t* d_handles, uint64_t* d_end,
                             uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* FilterBlockBuilder for every table at once.  With fi(b) = offset(b) >> 11
 * over a table's data handles (d_data_handles, relative) and fi(end) =
 * d_data_end[t] >> 11, the blocks of a table that share one fi form one filter
 * over their keys [d_block_first[first], d_block_first[last + 1]); it takes
 * slot fi of the table's offset array, the slots up to the next filter's
 * repeat the running size of the filter data, and the array has
 * fi(end) + (fi(end) == fi(last block) ? 1 : 0) slots (none without a block).
 *
 * d_out == NULL: only d_filter_size[t] (the filter block's size: filter data,
 * offset array, array offset, kFilterBaseLg) and d_filter_count[t] (its
 * filters) are written.  Otherwise also
 *   d_filter_first[sum of counts + 1], d_filter_out[sum of counts]
 *                           in the shape lsbm_bloom_build_dev takes, the
 *                           filters of all tables in order (they tile the
 *                           entries); filter_out is an offset into d_out
 *   the table's trailer     (offset array, array offset, kFilterBaseLg) at its
 *                           place in the window d_out[d_out_handles[2t],
 *                           + d_out_handles[2t + 1]), the filter block's
 * and lsbm_bloom_build_dev then writes every filter of every table.
 * LSBM_BUILD_NO_ROOM: the window is smaller than the block or not inside
 * out_size, or filters_cap is smaller than the sum of the counts; such a
 * table's filters have filter_out LSBM_TABLE_NO_PLACE and the caller keeps
 * them from lsbm_bloom_build_dev (which has no bounds of its own). */
int lsbm_filter_layout_dev(const uint64_t* d_block_first, const uint64_t* d_table_block_first, uint64_t n_blocks,
                           uint64_t n_tables, const uint64_t* d_data_handles, const uint64_t* d_data_end,
                           int bits_per_key, uint64_t* d_filter_size, uint64_t* d_filter_count,
                           uint64_t* d_filter_first, uint64_t* d_filter_out, uint64_t filters_cap, uint8_t* d_out,
                           uint64_t out_size, const uint64_t* d_out_handles, uint32_t* d_status, void* d_scratch,
                           uint64_t scratch_bytes, void* stream);

/* One metaindex block per table: with d_filter_size the single entry
 * "filter.leveldb.BuiltinBloomFilter" -> BlockHandle{d_data_end[t],
 * d_filter_size[t]}, with d_filter_size == NULL the 8-byte empty block.
 * d_sizes[t] is always written; with d_out the block goes to the start of
 * d_out[d_out_handles[2t], + d_out_handles[2t + 1]) (LSBM_BUILD_NO_ROOM where
 * it does not fit). */
int lsbm_metaindex_build_dev(const uint64_t* d_data_end, const uint64_t* d_filter_size, uint64_t n_tables,
                             uint64_t* d_sizes, uint8_t* d_out, uint64_t out_size, const uint64_t* d_out_handles,
                             uint32_t* d_status, void* stream);

/* Footers and placement.  Every table has tail_per_table (2 or 3) blocks after
 * its data blocks, the last two of them the metaindex and the index block;
 * d_tail_handles[2 tail_per_table n_tables] and d_tail_end[n_tables] are the
 * second lsbm_table_pack_plan_dev call's.  Per table
 *   d_table_size[t] = d_tail_end[t] + 48
 *   the footer (both handles, relative; padding; magic) at
 *                     d_arena[d_table_base[t] + d_tail_end[t], + 48)
 * LSBM_BUILD_NO_ROOM where [d_table_base[t], + d_table_size[t]) is not inside
 * arena_size: no footer is written.  Every handle is emitted with its table's
 * base added, as lsbm_block_pack_dev and lsbm_sst_seal_dev take them:
 * d_abs_data_handles[2 n_blocks], d_abs_tail_handles[2 tail_per_table n_tables]. */
int lsbm_table_place_dev(const uint64_t* d_data_handles, uint64_t n_blocks, const uint64_t* d_table_block_first,
                         const uint64_t* d_tail_handles, uint32_t tail_per_table, const uint64_t* d_tail_end,
                         const uint64_t* d_table_base, uint64_t n_tables, uint8_t* d_arena, uint64_t arena_size,
                         uint64_t* d_table_size, uint64_t* d_abs_data_handles, uint64_t* d_abs_tail_handles,
                         uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* lsbm_memtable_sort_dev over the memtables of one log.  Segment s is the
 * entries [d_seg_first[s], d_seg_first[s + 1]); the segments tile [0,
 * n_entries) (d_seg_first has n_segs + 1 words, begins with 0, never decreases,
 * ends with n_entries; empty segments are allowed).  Within a segment the
 * order is the memtable's (user key ascending, tag descending, the later of
 * equal internal keys first); the segments stay in input order and never
 * interleave.  Outputs as lsbm_memtable_sort_dev's, so lsbm_merge_gather_dev
 * gathers them: d_source[n_entries], d_out_key_offsets[n_entries + 1],
 * d_counts[2] = {n_entries, key bytes}, d_status[1].  LSBM_MERGE_BAD_INPUT with
 * d_counts = {0, 0}, d_source untouched: a d_seg_first that does not tile, or
 * a key shorter than 8 bytes or outside keys_size. */
uint64_t lsbm_memtable_sort_segments_scratch_bytes(uint64_t n_entries, uint64_t n_segs);
int lsbm_memtable_sort_segments_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                                    uint64_t n_entries, const uint64_t* d_seg_first, uint64_t n_segs,
                                    uint64_t* d_source, uint64_t* d_out_key_offsets, uint64_t* d_counts,
                                    uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_TABLE_WRITE_H_ */
