/*
 * lsbm_write.h -- C ABI of the MI355X (gfx950) batched DB::Write: the queued
 * writers' ops encoded as WriteBatch reps, cut into groups by
 * DBImpl::BuildBatchGroup's rule, and the groups' reps framed as log records,
 * for all writers of a queue in one launch sequence.  Implemented by
 * lsbm_amd/liblsbm_crc32c.so with the conventions of include/lsbm_memtable.h
 * and include/lsbm_iter.h: extern "C", device pointers and an explicit stream
 * (`void*` hipStream_t), calls only enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   common/write_batch.cc:98-109     WriteBatch::Put, Delete
 *   util/coding.cc                   PutVarint32, PutLengthPrefixedSlice
 *                                    -> lsbm_write_sizes_dev, lsbm_write_build_dev
 *   lsbm/db_impl.cc:1396-1441        DBImpl::BuildBatchGroup
 *                                    -> lsbm_write_group_dev
 *   common/write_batch.cc:141-145    WriteBatchInternal::Append
 *   common/write_batch.cc:86-96      SetSequence / SetCount
 *   lsbm/db_impl.cc:1338-1343, 1372  DBImpl::Write's sequence arithmetic
 *                                    -> lsbm_write_build_dev
 *   common/log_writer.cc:27-100      log::Writer::AddRecord, EmitPhysicalRecord
 *                                    (the CRC bytes are lsbm_log_seal_dev's)
 *                                    -> lsbm_log_frame_plan_dev, lsbm_log_frame_dev
 *
 * A call models n_writers writers already queued in writers_ in the given
 * order, each with a non-NULL batch.  Ops are in the shape the other engines
 * use: d_types[n_ops] (1 Put, 0 Delete), user keys as d_keys +
 * d_key_offsets[n_ops + 1], values as {offset, length} pairs into a value
 * image (ignored for a Delete); d_batch_first[n_writers + 1] is the op range
 * of each writer's batch (an empty batch is legal: 12 bytes).  n_ops and
 * n_writers are below 2^31; every size, cap and log offset below 2^62.
 *
 * Every call has one device status word, d_status[0]: LSBM_MERGE_OK,
 * LSBM_MERGE_NO_ROOM (a cap is too small) or LSBM_MERGE_BAD_INPUT.  On either
 * error no other output changes.  LSBM_MERGE_BAD_INPUT: a type byte above 1; a
 * key or value length of 2^32 or more (the reference would truncate it in
 * PutVarint32); offsets that decrease or pass their image; a d_batch_first or
 * d_group_first that is not monotone from 0 to its end; running sums, plans or
 * cuts that are not the ones an earlier step wrote for these inputs; a
 * log_offset with 0 < log_offset % 32768 < 7 (no log the reference wrote has
 * that size).  Nothing is written outside the stated sizes.  Where pointers
 * and sizes show an overlap between an output and an input, or between two
 * outputs, the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_WRITE_H_
#define LSBM_WRITE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

/* Device scratch lsbm_write_sizes_dev and lsbm_write_group_dev need (bytes; the
 * caller allocates, 8-byte aligned, contents are the call's own). */
uint64_t lsbm_write_scratch_bytes(uint64_t n_ops, uint64_t n_writers);

/* Step 1.  op_bytes(j) = 1 + varint_len(klen) + klen, plus varint_len(vlen) +
 * vlen for a Put.
 *   d_op_sum[n_ops + 1]        the exclusive running sum of op_bytes
 *   d_batch_sum[n_writers + 1] the exclusive running sum of
 *                              WriteBatchInternal::ByteSize(batch w) = 12 + its
 *                              ops' bytes: 12 w + d_op_sum[d_batch_first[w]] */
int lsbm_write_sizes_dev(const uint8_t* d_types, const uint64_t* d_key_offsets, uint64_t keys_size,
                         const uint64_t* d_values, uint64_t value_image_size, uint64_t n_ops,
                         const uint64_t* d_batch_first, uint64_t n_writers, uint64_t* d_op_sum, uint64_t* d_batch_sum,
                         uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Step 2.  BuildBatchGroup, run until the queue has drained.  A group led by
 * writer f, with size_f its ByteSize, has max_size = size_f <= 131072 ? size_f
 * + 131072 : 1048576 and takes the following writers w in order until
 * sync[w] && !sync[f] (checked first) or the running size += ByteSize(w)
 * exceeds max_size (equal still joins; every batch's own 12-byte header counts).
 *   d_batch_sum[n_writers + 1] running sums of ByteSize (any start; every
 *                              ByteSize at least 12, or LSBM_MERGE_BAD_INPUT)
 *   d_sync[n_writers]          nonzero: WriteOptions::sync; NULL: all false
 *   d_group_first[groups_cap + 1]  the leaders, then n_writers
 *   d_group_sync[groups_cap]       sync of each leader
 *   d_n_groups[0]              more than groups_cap: LSBM_MERGE_NO_ROOM */
int lsbm_write_group_dev(const uint64_t* d_batch_sum, uint64_t n_writers, const uint8_t* d_sync,
                         uint64_t* d_group_first, uint8_t* d_group_sync, uint64_t groups_cap, uint64_t* d_n_groups,
                         uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Step 3.  Group g's rep: fixed64(sequence_g) || fixed32(count_g) || the
 * encodings of all ops of its writers in order (what the group's leader passes
 * to log_->AddRecord and InsertInto, whichever branch BuildBatchGroup took);
 * sequence_0 = last_sequence + 1, sequence_{g+1} = sequence_g + count_g.  The
 * reps lie back to back in d_reps, group g's at 12 g + d_op_sum[its first op].
 * d_group_first may be any cut of the writers (n_groups + 1 slots, strictly
 * increasing from 0 to n_writers); d_op_sum is lsbm_write_sizes_dev's.
 *   d_reps[reps_cap]           12 n_groups + d_op_sum[n_ops] bytes; a smaller
 *                              cap: LSBM_MERGE_NO_ROOM
 *   d_records[2 n_groups]      {offset, length} of each rep: what
 *                              lsbm_wb_scan_dev / lsbm_log_frame_plan_dev take
 *   d_seq_counts[2 n_groups]   {sequence_g, count_g}
 *   d_last_sequence[0]         last_sequence + n_ops */
int lsbm_write_build_dev(const uint8_t* d_types, const uint8_t* d_keys, uint64_t keys_size,
                         const uint64_t* d_key_offsets, const uint8_t* d_value_image, uint64_t value_image_size,
                         const uint64_t* d_values, uint64_t n_ops, const uint64_t* d_batch_first, uint64_t n_writers,
                         const uint64_t* d_op_sum, const uint64_t* d_group_first, uint64_t n_groups,
                         uint64_t last_sequence, uint8_t* d_reps, uint64_t reps_cap, uint64_t* d_records,
                         uint64_t* d_seq_counts, uint64_t* d_last_sequence, uint32_t* d_status, void* stream);

/* Step 4.  AddRecord over n_records records of image_size-bounded {offset,
 * length} pairs (a length of 0 is legal), the first appended at file offset
 * log_offset.
 *   d_frag_first[n_records + 1]  the running count of physical records
 *   d_rec_start[n_records + 1]   the file offset of each record's first header
 *                                (after the zero trailer of a block with fewer
 *                                than 7 bytes left); slot n_records: the end
 *                                offset of the log */
int lsbm_log_frame_plan_dev(uint64_t image_size, const uint64_t* d_records, uint64_t n_records, uint64_t log_offset,
                            uint64_t* d_frag_first, uint64_t* d_rec_start, uint32_t* d_status, void* stream);

/* Step 5.  The appended bytes [log_offset, end) into d_out, whose byte 0 is file
 * offset log_offset: leading zero padding if the log ended within 6 bytes of a
 * block end, every header's length and type bytes with the CRC bytes 0,
 * payload fragments copied from d_image, zero trailers.  d_frag_first and
 * d_rec_start are lsbm_log_frame_plan_dev's for the same records and offset.
 *   d_out[out_cap]           end - log_offset bytes; smaller: LSBM_MERGE_NO_ROOM
 *   d_headers[headers_cap]   d_frag_first[n_records] offsets relative to
 *                            d_out, in file order: what lsbm_log_seal_dev takes */
int lsbm_log_frame_dev(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n_records,
                       uint64_t log_offset, const uint64_t* d_frag_first, const uint64_t* d_rec_start, uint8_t* d_out,
                       uint64_t out_cap, uint64_t* d_headers, uint64_t headers_cap, uint32_t* d_status, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_WRITE_H_ */
