/*
 * lsbm_manifest.h -- C ABI of the MI355X (gfx950) batched VersionEdit: the
 * records of a MANIFEST decoded (VersionEdit::DecodeFrom) and encoded
 * (VersionEdit::EncodeTo) many at once, the entries of one long record found
 * in parallel.  Implemented by lsbm_amd/liblsbm_crc32c.so with the
 * conventions of include/lsbm_log_read.h: extern "C", device pointers and an
 * explicit stream (`void*` hipStream_t), calls only enqueue and allocate
 * nothing, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   lsbm/version_edit.cc:137-251  VersionEdit::DecodeFrom
 *                                 -> lsbm_edit_decode_plan_dev, lsbm_edit_decode_emit_dev
 *   lsbm/version_edit.cc:51-114   VersionEdit::EncodeTo
 *                                 -> lsbm_edit_encode_plan_dev, lsbm_edit_encode_emit_dev
 *
 * Records are {offset, length} pairs into a device image, what
 * lsbm_log_read_emit_dev writes and lsbm_frame_* take; offsets need not
 * ascend.  Offsets are below 2^62.  The records of one decode call hold fewer
 * than 2^32 - 64 bytes together.
 *
 * An edit's fields are LSBM_EDIT_FIELD_WORDS uint64 words:
 *   [LSBM_EDIT_HAS]           bits: 1 comparator, 2 log number, 4 previous log
 *                             number, 8 next file number, 16 last sequence,
 *                             32 write cursor
 *   [LSBM_EDIT_READ_HAS]      bit i: read cursor i
 *   [LSBM_EDIT_LOG .. + 4]    log number, previous log number, next file
 *                             number, last sequence, write cursor
 *   [LSBM_EDIT_READ .. + 3]   read cursors
 *   [LSBM_EDIT_CMP_OFF], [LSBM_EDIT_CMP_LEN]   the comparator's name: decode
 *                             gives it in d_image, encode takes it in d_names
 * New files are LSBM_EDIT_NEW_WORDS words {record, type, level, number,
 * file_size}; key 2j of d_keys / d_key_offsets[2 n_new + 1] is file j's
 * smallest and key 2j + 1 its largest.  Deleted files are
 * LSBM_EDIT_DEL_WORDS words {record, type, level, number}.  Items are flat,
 * in record order; d_new_first[n + 1] and d_del_first[n + 1] are the running
 * counts.
 *
 * A record's verdict is 0 (OK) or the reference's message:
 *   1 comparator name, 2 log number, 3 previous log number, 4 next file
 *   number, 5 last sequence number, 6 deleted file, 7 new-file entry, 8 write
 *   cursor, 9 read cursor, 10 unknown tag, 11 invalid tag
 * or one of two codes for input on which the reference's behaviour is
 * undefined: 12 a deleted-file or new-file group that parses completely but
 * has type >= 4, 13 a read-cursor group whose index parses and is >= 4.  A
 * record with a verdict other than 0 has no items and no fields.
 *
 * Every call has one device status word, d_status[0]: LSBM_MERGE_OK,
 * LSBM_MERGE_NO_ROOM (a cap is too small) or LSBM_MERGE_BAD_INPUT.  On either
 * error no other output changes.  Nothing is written outside the stated
 * sizes.  Where pointers and sizes show an overlap between an output and an
 * input or between two outputs, the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_MANIFEST_H_
#define LSBM_MANIFEST_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_EDIT_HAS 0
#define LSBM_EDIT_READ_HAS 1
#define LSBM_EDIT_LOG 2
#define LSBM_EDIT_READ 7
#define LSBM_EDIT_CMP_OFF 11
#define LSBM_EDIT_CMP_LEN 12
#define LSBM_EDIT_FIELD_WORDS 13
#define LSBM_EDIT_NEW_WORDS 5
#define LSBM_EDIT_DEL_WORDS 4

/* Device scratch (bytes; the caller allocates, 8-byte aligned).  The plan of
 * either pair leaves its result in the scratch and the emit takes it from
 * there: the same scratch and the same inputs, untouched in between. */
uint64_t lsbm_edit_decode_scratch_bytes(uint64_t n, uint64_t span_cap);
uint64_t lsbm_edit_encode_scratch_bytes(uint64_t n, uint64_t n_del, uint64_t n_new);

/* Decode, first call: finds the entries of n records and writes
 *   d_verdict[n], d_fields[LSBM_EDIT_FIELD_WORDS n], d_new_first[n + 1],
 *   d_del_first[n + 1], d_totals[3] = {n_new, n_deleted, key bytes}
 * span_cap bounds the records' lengths summed and longest_cap the longest
 * record: a batch that exceeds either is LSBM_MERGE_NO_ROOM.  A record that
 * reaches outside the image is LSBM_MERGE_BAD_INPUT. */
int lsbm_edit_decode_plan_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n,
                              uint64_t span_cap, uint64_t longest_cap, uint32_t* d_verdict, uint64_t* d_fields,
                              uint64_t* d_new_first, uint64_t* d_del_first, uint64_t* d_totals, uint32_t* d_status,
                              void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Decode, second call: the items written out, with caps sized from d_totals.
 *   d_new_items[LSBM_EDIT_NEW_WORDS new_cap], d_key_offsets[2 new_cap + 1],
 *   d_keys[keys_cap], d_del_items[LSBM_EDIT_DEL_WORDS del_cap]
 * A cap below its total: LSBM_MERGE_NO_ROOM.  2 n_new + 1 offsets are written. */
int lsbm_edit_decode_emit_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n,
                              uint64_t span_cap, uint64_t* d_new_items, uint64_t new_cap, uint64_t* d_key_offsets,
                              uint8_t* d_keys, uint64_t keys_cap, uint64_t* d_del_items, uint64_t del_cap,
                              uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Encode, first call: sizes n edits and writes d_records[2 n] = {out_at +
 * offset, length} and d_totals[1] = {bytes}.  Every edit is written with its
 * write cursor and four read cursors, as the reference writes them.
 * LSBM_MERGE_BAD_INPUT: the deleted files of an edit are not strictly
 * ascending by (type, level, number); its new files descend in type; a type
 * or level is 4 or more; an item's record is not the edit that lists it;
 * first arrays or key offsets that decrease or pass their buffer; a key or
 * name of 2^32 bytes or more. */
int lsbm_edit_encode_plan_dev(const uint64_t* d_fields, const uint8_t* d_names, uint64_t names_size, uint64_t n,
                              const uint64_t* d_del_first, const uint64_t* d_del_items, uint64_t n_del,
                              const uint64_t* d_new_first, const uint64_t* d_new_items, uint64_t n_new,
                              const uint8_t* d_keys, const uint64_t* d_key_offsets, uint64_t keys_size,
                              uint64_t out_at, uint64_t* d_records, uint64_t* d_totals, uint32_t* d_status,
                              void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Encode, second call: the edits' bytes in d_image[out_at, out_at + bytes).
 * out_cap below the plan's bytes: LSBM_MERGE_NO_ROOM. */
int lsbm_edit_encode_emit_dev(const uint64_t* d_fields, const uint8_t* d_names, uint64_t names_size, uint64_t n,
                              const uint64_t* d_del_first, const uint64_t* d_del_items, uint64_t n_del,
                              const uint64_t* d_new_first, const uint64_t* d_new_items, uint64_t n_new,
                              const uint8_t* d_keys, const uint64_t* d_key_offsets, uint64_t keys_size,
                              uint8_t* d_image, uint64_t image_size, uint64_t out_at, uint64_t out_cap,
                              uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_MANIFEST_H_ */
