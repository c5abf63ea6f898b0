/*
 * lsbm_log_read.h -- C ABI of the MI355X (gfx950) batched log::Reader: the
 * loop `while (reader.ReadRecord(&record, &scratch))` of DBImpl::RecoverLogFile
 * and VersionSet::Recover over a log image in device memory, with every
 * record, every LastRecordOffset() and every Reporter::Corruption call in the
 * reference's order.  Implemented by lsbm_amd/liblsbm_crc32c.so with the
 * conventions of include/lsbm_write.h: extern "C", device pointers and an
 * explicit stream (`void*` hipStream_t), calls only enqueue, LSBM_* status
 * codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   common/log_reader.cc:35-57    Reader::SkipToInitialBlock
 *   common/log_reader.cc:179-256  Reader::ReadPhysicalRecord
 *                                 -> lsbm_log_read_walk_dev (lengths),
 *                                    lsbm_log_verify_dev (CRCs, lsbm_crc32c.h),
 *                                    lsbm_log_read_plan_dev (drops, the skip)
 *   common/log_reader.cc:59-162   Reader::ReadRecord
 *   common/log_reader.cc:172-177  Reader::ReportDrop's filter
 *                                 -> lsbm_log_read_plan_dev, lsbm_log_read_emit_dev
 *
 * The reader is Reader(file, reporter, checksum = true, initial_offset).  The
 * log is d_image[log_at, log_at + log_bytes); header offsets, initial_offset,
 * last_record_offset and the stop offset count from the log's first byte.
 * Assembled records go to the side area d_image[side_at, side_at + side_cap)
 * of the same image, so d_records' offsets are offsets in d_image, which
 * lsbm_wb_scan_dev takes as they are.  Offsets and sizes are below 2^62.
 *
 * Reading covers the blocks from SkipToInitialBlock's block on:
 * lsbm_log_read_blocks(log_bytes, initial_offset) of them, the first one
 * block number (initial_offset - initial_offset % 32768) / 32768, plus one if
 * initial_offset % 32768 > 32762.
 *
 * Every call has one device status word, d_status[0]: LSBM_MERGE_OK,
 * LSBM_MERGE_NO_ROOM (a cap is too small) or LSBM_MERGE_BAD_INPUT (block or
 * header arrays that are not the walk's for this image).  On either error no
 * other output changes.  Nothing is written outside the stated sizes.  Where
 * pointers and sizes show an overlap between an output and an input or
 * between two outputs, or the side area and the log share a byte, the call
 * returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_LOG_READ_H_
#define LSBM_LOG_READ_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

/* Device scratch that is enough for every step on any log of log_bytes
 * (bytes; the caller allocates, 8-byte aligned).  It assumes a header every 7
 * bytes; lsbm_log_read_plan_scratch_bytes is the figure for a known header
 * count.  lsbm_log_read_plan_dev leaves its plan in the scratch and
 * lsbm_log_read_emit_dev takes it from there: the same scratch, untouched in
 * between. */
uint64_t lsbm_log_read_scratch_bytes(uint64_t log_bytes);
uint64_t lsbm_log_read_plan_scratch_bytes(uint64_t n_headers, uint64_t n_blocks);
uint64_t lsbm_log_read_blocks(uint64_t log_bytes, uint64_t initial_offset);

/* Step 1.  ReadPhysicalRecord's walk of every block from its own start, every
 * CRC assumed good: a header is parsed where 7 bytes or more are left, its
 * 7 + length fit in the rest of the block, and it is not type 0 with length 0.
 *   d_block_first[n_blocks + 1]  the running count of headers parsed
 *   d_block_end[2 n_blocks]      {how the walk ended, bytes left}: 0 ran out
 *                                (0 left), 1 trailer (1..6 left in a whole
 *                                block), 2 bad record length, 3 zero header,
 *                                4 truncated (1..6 left in the short last block)
 *   d_headers[headers_cap]       the header offsets in file order: what
 *                                lsbm_log_verify_dev(d_image + log_at,
 *                                log_bytes, ...) takes.  NULL: count only
 *   d_n_headers[0]               more than headers_cap: LSBM_MERGE_NO_ROOM
 * Scratch: 8 (3 n_blocks + 1) bytes. */
int lsbm_log_read_walk_dev(const uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes,
                           uint64_t initial_offset, uint64_t* d_block_first, uint64_t* d_block_end, uint64_t n_blocks,
                           uint64_t* d_headers, uint64_t headers_cap, uint64_t* d_n_headers, uint32_t* d_status,
                           void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Step 2 (after lsbm_log_verify_dev has filled d_ok[n_headers]).  Cuts each
 * block at its first failed CRC, applies the initial_offset skip and
 * ReportDrop's filter, runs ReadRecord's state machine and finds the stop:
 * the end of the file or the first surviving record of type 5.
 *   d_totals[4]   {n_records, n_events, side_bytes, stop offset (the type-5
 *                 header's, or log_bytes)}
 * The walk's three arrays are verified against the image:
 * LSBM_MERGE_BAD_INPUT if they are not what step 1 writes for it. */
int lsbm_log_read_plan_dev(const uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes,
                           uint64_t initial_offset, const uint64_t* d_block_first, const uint64_t* d_block_end,
                           uint64_t n_blocks, const uint64_t* d_headers, uint64_t n_headers, const uint8_t* d_ok,
                           uint64_t* d_totals, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                           void* stream);

/* Step 3.  The plan written out, with the same log and counts as step 2.
 *   d_records[2 records_cap]          {offset in d_image, length}: an
 *                                     unfragmented record is its payload in
 *                                     place, a fragmented one lies in the side
 *                                     area, back to back in record order
 *   d_last_record_offset[records_cap] LastRecordOffset() after each record
 *   d_events[4 events_cap]            {records returned before the call,
 *                                     bytes, reason, arg} of each
 *                                     Reporter::Corruption call.  Reasons:
 *                                     1 bad record length, 2 checksum mismatch,
 *                                     3 truncated record at end of file,
 *                                     4 / 5 / 6 partial record without
 *                                     end(1) / (2) / (3), 7 / 8 missing start
 *                                     of fragmented record(1) / (2), 9 error in
 *                                     middle of record, 10 unknown record type
 *                                     (arg: the type, a char widened to
 *                                     unsigned int)
 * A cap below the plan's total (records, events, side bytes):
 * LSBM_MERGE_NO_ROOM.  Only side_bytes bytes of the side area are written. */
int lsbm_log_read_emit_dev(uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes,
                           uint64_t initial_offset, uint64_t n_blocks, uint64_t n_headers, uint64_t side_at,
                           uint64_t side_cap, uint64_t* d_records, uint64_t records_cap,
                           uint64_t* d_last_record_offset, uint64_t* d_events, uint64_t events_cap, uint32_t* d_status,
                           void* d_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_LOG_READ_H_ */
