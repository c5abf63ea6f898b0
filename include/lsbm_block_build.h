/*
 * lsbm_block_build.h -- C ABI of the MI355X (gfx950) batched SSTable block
 * builder: BlockBuilder::Add / Finish of lsbm's table/block_builder.cc, the
 * flush rule of TableBuilder::Add and the index block of TableBuilder, for
 * many blocks in one launch.  Implemented by lsbm_amd/liblsbm_crc32c.so with
 * the conventions of include/lsbm_block.h: extern "C", device pointers and an
 * explicit stream (`void*` hipStream_t), calls only enqueue, LSBM_* status
 * codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   table/block_builder.cc:57-107   BlockBuilder::Finish / Add
 *                                   -> lsbm_block_build_dev
 *   table/block_builder.cc:51-55    CurrentSizeEstimate
 *   table/table_builder.cc:108-141  TableBuilder::Add's flush rule
 *                                   -> lsbm_block_plan_dev
 *   table/table_builder.cc:120-127, :292-299  the index entries
 *   util/comparator.cc:29-65        Bytewise FindShortestSeparator / FindShortSuccessor
 *   common/dbformat.cc:68-99        InternalKeyComparator's, with the tag
 *                                   PackSequenceAndType(kMaxSequenceNumber, kValueTypeForSeek)
 *   table/format.cc:15-21           BlockHandle::EncodeTo
 *                                   -> lsbm_index_block_build_dev
 *
 * Entries are what lsbm_block_decode_dev writes:
 *   key e   = d_keys[d_key_offsets[e], d_key_offsets[e+1])   (keys_size bytes)
 *   value e = d_value_image[d_values[2e], + d_values[2e+1])  (value_image_size bytes)
 * Keys need not be sorted (the reference only asserts order).
 *
 * No byte outside the key buffer and the value image is read, and no byte
 * outside a block's window is written.  Outputs must not alias inputs: where
 * pointers and sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_BLOCK_BUILD_H_
#define LSBM_BLOCK_BUILD_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h" /* LSBM_CMP_*, LSBM_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Per-block (build) and per-table (plan, index) status.  A block or table
 * with several findings reports the largest code.  Where the reference has no
 * verdict:
 *   LSBM_BUILD_NO_ROOM    the window is smaller than the block; the window's
 *                         contents are unspecified
 *   LSBM_BUILD_BAD_INPUT  key offsets decrease or pass keys_size; a value
 *                         slice is not wholly inside the value image;
 *                         block_first / table_first / table_block_first
 *                         decrease or pass their limit; a window is not wholly
 *                         inside the output; an index entry is asked of a
 *                         block without entries; under LSBM_CMP_INTERNAL_KEY a
 *                         key shorter than 8 bytes (the reference asserts).
 *                         Nothing is written for that block or table.
 *   LSBM_BUILD_TOO_LARGE  the block's contents would reach 2^32 bytes (the
 *                         reference's 32-bit restart offsets wrap there).
 *                         Nothing is written for it. */
#define LSBM_BUILD_OK 0u
#define LSBM_BUILD_NO_ROOM 1u
#define LSBM_BUILD_BAD_INPUT 2u
#define LSBM_BUILD_TOO_LARGE 3u

/* Per-run status of the compaction merge that feeds the builder
 * (include/lsbm_merge.h, which says what each means). */
#define LSBM_MERGE_OK 0u
#define LSBM_MERGE_NO_ROOM 1u
#define LSBM_MERGE_BAD_INPUT 2u
#define LSBM_MERGE_UNSORTED 3u

/* Device scratch lsbm_block_plan_dev needs for n_entries entries in n_tables
 * tables (bytes; the caller allocates, contents are the call's own). */
uint64_t lsbm_block_plan_scratch_bytes(uint64_t n_entries, uint64_t n_tables);

/* Where blocks end: TableBuilder::Add's rule.  Table t owns entries
 * [d_table_first[t], d_table_first[t+1]); the tables tile a contiguous range
 * (with a d_table_first that does not, the tables in error get
 * LSBM_BUILD_BAD_INPUT and no blocks, and the plan of the others is
 * unspecified).  After each Add the block is flushed when
 * CurrentSizeEstimate() = buffer bytes + 4 x restart points + 4 >= block_size;
 * a table's last block is what is left; a table without entries has no
 * blocks.  Reads keys and value lengths (d_values[2e+1]), never a value byte.
 * Outputs, dense and in table order:
 *   d_block_first[b]        first entry of block b; blocks_cap + 1 slots, the
 *                           slot after the last block holds the end
 *   d_block_bytes[b]        the size Finish() will return (blocks_cap slots;
 *                           unspecified for a block of a table in error)
 *   d_table_block_first[t]  running block count, n_tables + 1 slots; the last
 *                           one is the true total also when it exceeds
 *                           blocks_cap: then nothing is written past the cap
 *                           and the caller retries
 *   d_status[t]             LSBM_BUILD_* per table
 * A block that holds an entry of 2^32 - 1 bytes or more is LSBM_BUILD_TOO_LARGE. */
int lsbm_block_plan_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                        const uint64_t* d_values, uint64_t n_entries, const uint64_t* d_table_first,
                        uint64_t n_tables, uint64_t block_size, uint32_t restart_interval,
                        uint64_t* d_block_first, uint64_t* d_block_bytes, uint64_t blocks_cap,
                        uint64_t* d_table_block_first, uint32_t* d_status, void* d_scratch,
                        uint64_t scratch_bytes, void* stream);

/* BlockBuilder::Add for entries [d_block_first[b], d_block_first[b+1]) and
 * Finish, for n_blocks blocks.  Block b is written at the start of its window
 * d_out[d_out_handles[2b], + d_out_handles[2b+1]) (windows as
 * table.layout_blocks lays them out; they must not overlap each other).
 *   d_built_bytes[b]  the block's true size, also with LSBM_BUILD_NO_ROOM
 *                     (0 with BAD_INPUT / TOO_LARGE); may be NULL
 *   d_status[b]       LSBM_BUILD_* per block
 * A block without entries is Finish() of a fresh builder: 8 bytes. */
int lsbm_block_build_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                         const uint64_t* d_values, const uint8_t* d_value_image, uint64_t value_image_size,
                         uint64_t n_entries, const uint64_t* d_block_first, uint64_t n_blocks,
                         uint32_t restart_interval, uint8_t* d_out, uint64_t out_size,
                         const uint64_t* d_out_handles, uint64_t* d_built_bytes, uint32_t* d_status,
                         void* stream);

/* One index block per table, restart interval 1 (table/table_builder.cc:70).
 * Table t owns data blocks [d_table_block_first[t], d_table_block_first[t+1]).
 * Entry i of a table: key FindShortestSeparator(last key of block i, first key
 * of block i+1), for the table's last block FindShortSuccessor(last key), under
 * cmp (LSBM_CMP_BYTEWISE / LSBM_CMP_INTERNAL_KEY); value BlockHandle::EncodeTo
 * of {d_data_handles[2b], d_data_handles[2b+1]}.  A table without blocks gets
 * the empty block (8 bytes).  Table t's block is written at the start of its
 * window d_out[d_out_handles[2t], + d_out_handles[2t+1]).  With d_out == NULL
 * only d_built_bytes[t] (and d_status[t]) are written: the sizes the caller
 * needs for the layout and the footer; d_out_handles may then be NULL. */
int lsbm_index_block_build_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                               uint64_t n_entries, const uint64_t* d_block_first, uint64_t n_blocks,
                               const uint64_t* d_table_block_first, uint64_t n_tables,
                               const uint64_t* d_data_handles, int cmp, uint8_t* d_out, uint64_t out_size,
                               const uint64_t* d_out_handles, uint64_t* d_built_bytes, uint32_t* d_status,
                               void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_BLOCK_BUILD_H_ */
