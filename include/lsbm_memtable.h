/*
 * lsbm_memtable.h -- C ABI of the MI355X (gfx950) memtable flush: the log's
 * WriteBatch records decoded into internal-key entries and put into the
 * memtable's iteration order, for all records of a memtable in one launch
 * sequence.  Implemented by lsbm_amd/liblsbm_crc32c.so with the conventions
 * of include/lsbm_merge.h: extern "C", device pointers and an explicit stream
 * (`void*` hipStream_t), calls only enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   common/write_batch.cc:42-80    WriteBatch::Iterate
 *   util/coding.cc:112-129         GetVarint32Ptr
 *                                  -> lsbm_wb_scan_dev, lsbm_wb_decode_dev
 *   common/write_batch.cc:112-134  MemTableInserter, InsertInto
 *   common/memtable.cc:83-107      MemTable::Add (the internal key)
 *   lsbm/db_impl.cc:456-461        RecoverLogFile's max_sequence
 *                                  -> lsbm_wb_decode_dev
 *   common/skiplist.h:334-367      SkipList::Insert under the memtable's
 *                                  KeyComparator, and the iteration it gives
 *                                  -> lsbm_memtable_sort_dev
 *
 * A record is image[records[2i], records[2i] + records[2i+1]): one
 * WriteBatch::rep_, that is one logical log record.  The pair may point into a
 * log image at the payload after a physical record's 7-byte header; a record
 * that spans fragments is assembled by the caller first.
 *
 * The entries are what lsbm_block_decode_dev writes (keys + key_offsets and
 * {offset, length} value slices into the image), so lsbm_block_plan_dev,
 * lsbm_bloom_build_dev and lsbm_merge_plan_dev / _gather_dev read them as they
 * are.  No byte outside the image is read, nothing is written outside the
 * outputs' stated sizes.  Outputs must not alias inputs: where pointers and
 * sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_MEMTABLE_H_
#define LSBM_MEMTABLE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

/* Per-record status of scan and decode.  The walk stops at its first error, as
 * the reference's does; the entries before it count. */
#define LSBM_WB_OK 0u
#define LSBM_WB_TOO_SMALL 1u   /* length < 12: RecoverLogFile's "log record too small"; no entries */
#define LSBM_WB_BAD_PUT 2u     /* Corruption("bad WriteBatch Put") */
#define LSBM_WB_BAD_DELETE 3u  /* Corruption("bad WriteBatch Delete") */
#define LSBM_WB_UNKNOWN_TAG 4u /* Corruption("unknown WriteBatch tag") */
#define LSBM_WB_WRONG_COUNT 5u /* Corruption("WriteBatch has wrong count"); every entry counts */
#define LSBM_WB_BAD_INPUT 6u   /* the pair reaches outside the image, or its length is >= 2^32; no entries */
#define LSBM_WB_NO_ROOM 7u     /* decode: the record's window is too small; its contents are unspecified */

/* the most entries lsbm_memtable_sort_dev takes */
#define LSBM_MEMTABLE_MAX_ENTRIES (1ull << 31)

/* WriteBatch::Iterate of n_records records.  Per record:
 *   d_counts[2i]     the entries whose handler->Put / Delete the reference
 *                    would have called before the end or the first error (a
 *                    Put whose value fails is not one of them): what its
 *                    memtable holds after InsertInto
 *   d_counts[2i+1]   bytes of their user keys (an entry's internal key has 8 more)
 *   d_status[i]      LSBM_WB_* */
int lsbm_wb_scan_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n_records,
                     uint64_t* d_counts, uint32_t* d_status, void* stream);

/* The same walk, written out.  Record i owns entries [d_entry_base[i],
 * d_entry_base[i+1]) and key bytes [d_key_base[i], d_key_base[i+1]) of the
 * outputs: both arrays are n_records + 1 long and are the running sums of a
 * prior scan's entries and of its user-key bytes + 8 per entry, as
 * lsbm_block_decode_dev takes its windows.  For entry j of a record whose
 * header holds sequence s, at e = d_entry_base[i] + j:
 *   key e = d_keys[d_key_offsets[e], d_key_offsets[e+1])
 *         = user key || fixed64((s + j) << 8 | type)
 *   d_values[2e], [2e+1] = {offset of the value bytes in the image, length};
 *         for a deletion length 0 and the offset just past the key
 * d_key_offsets has entries_cap + 1 slots; the slot after the last entry,
 * d_key_offsets[d_entry_base[n_records]], is set to d_key_base[n_records].
 * A record whose entries or key bytes do not fit its window, or whose window
 * passes keys_cap / entries_cap, gets LSBM_WB_NO_ROOM; nothing is written
 * outside the windows.
 *   d_max_sequence[0]  the largest s + count - 1 (count the header's, an int
 *                      as in the reference) over the records of at least 12
 *                      bytes inside the image; 0 without one */
int lsbm_wb_decode_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n_records,
                       const uint64_t* d_entry_base, const uint64_t* d_key_base, uint8_t* d_keys, uint64_t keys_cap,
                       uint64_t* d_key_offsets, uint64_t* d_values, uint64_t entries_cap, uint64_t* d_max_sequence,
                       uint32_t* d_status, void* stream);

/* Device scratch lsbm_memtable_sort_dev needs (bytes; the caller allocates,
 * 8-byte aligned, contents are the call's own). */
uint64_t lsbm_memtable_sort_scratch_bytes(uint64_t n_entries);

/* The memtable's iteration order over n_entries internal keys, as a
 * permutation in lsbm_merge_plan_dev's output shape (lsbm_merge_gather_dev
 * gathers it as it is):
 *   d_source[j]           the input entry at sorted position j
 *   d_out_key_offsets[j]  the running sum of the sorted keys' lengths
 *                         (n_entries + 1 slots)
 *   d_counts              {n_entries, key bytes}
 *   d_status[0]           LSBM_MERGE_OK or LSBM_MERGE_BAD_INPUT
 * Order: the user key (all but the last 8 bytes) bytewise ascending (memcmp,
 * then length); then the 64-bit little-endian tag descending; then, among
 * equal internal keys, the later entry first -- where a release build's
 * SkipList::Insert puts a key equal to one it holds.
 * A key shorter than 8 bytes, offsets that decrease or pass keys_size:
 * LSBM_MERGE_BAD_INPUT, d_counts = {0, 0}, and no key byte is read. */
int lsbm_memtable_sort_dev(const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
                           uint64_t n_entries, uint64_t* d_source, uint64_t* d_out_key_offsets, uint64_t* d_counts,
                           uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_MEMTABLE_H_ */
