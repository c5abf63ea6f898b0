/*
 * lsbm_block.h -- C ABI of the MI355X (gfx950) batched SSTable block reader:
 * Block::Iter of lsbm's table/block.cc for many blocks in one launch.
 * Implemented by lsbm_amd/liblsbm_crc32c.so, with the conventions of
 * include/lsbm_crc32c.h: extern "C", plain pointers and sizes, LSBM_* status
 * codes, never throws; `_dev` calls take device pointers and an explicit
 * stream (`void*` hipStream_t) and only enqueue.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   table/block.cc:23-41      Block::Block (size and restart-count checks)
 *   table/block.cc:111-132    DecodeEntry
 *   table/block.cc:267-270, :288-315  SeekToFirst / Next until !Valid
 *                             -> lsbm_block_scan_dev, lsbm_block_decode_dev
 *   table/block.cc:223-265    Block::Iter::Seek -> lsbm_block_seek_dev
 *   util/comparator.cc        BytewiseComparator -> LSBM_CMP_BYTEWISE
 *   common/dbformat.cc:50-66  InternalKeyComparator -> LSBM_CMP_INTERNAL_KEY
 *   table/format.cc:23-30     BlockHandle::DecodeFrom -> LSBM_SEEK_VALUE_IS_HANDLE
 *   table/table.cc:309-339    Table::InternalGet's index Seek, handle decode
 *                             and data-block Seek (lsbm_amd/block.py table_get)
 *
 * A block is image[handles[2i], handles[2i] + handles[2i+1]): the block
 * contents as BlockBuilder::Finish wrote them, without the 5-byte trailer.
 * Verdicts are the reference's, on malformed blocks too.  Defined by this
 * library, where the reference has no verdict:
 *   - a handle whose bytes are not wholly inside the image, or whose size is
 *     >= 2^32: "bad block contents";
 *   - an entry whose non_shared + value_length exceeds 2^32 - 1 (the
 *     reference's 32-bit sum wraps and it reads out of bounds): a bad entry;
 *   - under LSBM_CMP_INTERNAL_KEY a comparison that involves a key or a target
 *     shorter than 8 bytes (the reference asserts, common/dbformat.h:75-78)
 *     ends the query with "bad entry in block".
 * No byte outside [image, image + image_size) is read and none outside the
 * caller's windows is written.
 */
#ifndef LSBM_BLOCK_H_
#define LSBM_BLOCK_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_crc32c.h" /* LSBM_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* per-block status of scan and decode */
#define LSBM_BLOCK_OK 0u
#define LSBM_BLOCK_BAD_CONTENTS 1u /* Corruption("bad block contents") */
#define LSBM_BLOCK_BAD_ENTRY 2u    /* Corruption("bad entry in block"); the entries before it count */
#define LSBM_BLOCK_NO_ROOM 3u      /* decode: the block's window is too small; its contents are unspecified */

/* per-query state of seek */
#define LSBM_SEEK_VALID 0u
#define LSBM_SEEK_NOT_VALID 1u     /* !Valid(), status OK */
#define LSBM_SEEK_BAD_ENTRY 2u
#define LSBM_SEEK_BAD_CONTENTS 3u
#define LSBM_SEEK_BAD_HANDLE 4u    /* Corruption("bad block handle") */

#define LSBM_CMP_BYTEWISE 0
#define LSBM_CMP_INTERNAL_KEY 1

#define LSBM_SEEK_VALUE_IS_HANDLE 0x1u

/* SeekToFirst, then Next until !Valid, of n_blocks blocks.  Per block:
 *   d_counts[3i]     entries returned before the end or the first error
 *   d_counts[3i+1]   bytes of their fully expanded keys
 *   d_counts[3i+2]   bytes of their values
 *   d_status[i]      LSBM_BLOCK_OK / _BAD_CONTENTS / _BAD_ENTRY */
int lsbm_block_scan_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles,
                        uint64_t n_blocks, uint64_t* d_counts, uint32_t* d_status, void* stream);

/* The same walk, written out.  Block i owns entries [d_entry_base[i],
 * d_entry_base[i+1]) and key bytes [d_key_base[i], d_key_base[i+1]) of the
 * outputs (both arrays n_blocks + 1 long: running sums of a prior scan's
 * counts, as lsbm_snappy_uncompress_dev takes its windows).  For entry e:
 *   key e = d_keys[d_key_offsets[e], d_key_offsets[e+1])   (the layout
 *           lsbm_bloom_build_dev reads; d_key_offsets has entries_cap + 1 slots)
 *   d_values[2e], d_values[2e+1] = {absolute offset in the image, length}
 * A block whose entries or key bytes do not fit its window, or whose window
 * passes keys_cap / entries_cap, gets LSBM_BLOCK_NO_ROOM; nothing is written
 * outside the windows.  A window larger than needed leaves its unused key
 * offsets unwritten.  d_counts (as in scan) may be NULL. */
int lsbm_block_decode_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles,
                          uint64_t n_blocks, const uint64_t* d_entry_base, const uint64_t* d_key_base,
                          uint8_t* d_keys, uint64_t keys_cap, uint64_t* d_key_offsets, uint64_t* d_values,
                          uint64_t entries_cap, uint64_t* d_counts, uint32_t* d_status, void* stream);

/* NewIterator(cmp)->Seek(target) for n_queries lookups: block
 * image[handles[2q], + handles[2q+1]), target d_keys[key_offsets[q],
 * key_offsets[q+1]).  Per query:
 *   d_state[q]     LSBM_SEEK_*
 *   d_pos[q]       current_: the found entry's offset in the block; restarts_
 *                  when not valid (size - 4 for a block without restart
 *                  points, 0 for bad block contents)
 *   d_key_len[q]   length of the found key (0 unless an entry was found)
 *   d_value[2q], [2q+1]  {absolute offset in the image, length} of its value
 *                  (0, 0 unless an entry was found; LSBM_SEEK_BAD_HANDLE keeps
 *                  pos, key length and value of the entry whose value it is)
 * flags & LSBM_SEEK_VALUE_IS_HANDLE: a valid result's value is decoded as a
 * BlockHandle into d_handle_out[2q], [2q+1] ({0, 0} otherwise); a value that
 * does not decode sets LSBM_SEEK_BAD_HANDLE.  d_handle_out may be NULL
 * without the flag.
 * d_found (may be NULL): the found key is copied to
 * d_found[found_offsets[q], ...) if it fits the window up to
 * found_offsets[q+1]; d_key_len always holds the true length.  The window is
 * the walk's working copy: when the key does not fit, or no entry is found,
 * its contents are unspecified (nothing is written outside it). */
int lsbm_block_seek_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_handles,
                        const void* d_keys, const uint64_t* d_key_offsets, uint64_t n_queries, int cmp,
                        uint32_t flags, uint32_t* d_state, uint64_t* d_pos, uint64_t* d_key_len,
                        uint64_t* d_value, uint64_t* d_handle_out, uint8_t* d_found,
                        const uint64_t* d_found_offsets, uint64_t found_cap, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_BLOCK_H_ */
