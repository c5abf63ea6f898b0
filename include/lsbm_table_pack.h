/*
 * lsbm_table_pack.h -- C ABI of the MI355X (gfx950) table packer: the keep
 * rule of TableBuilder::WriteBlock and the file offsets that follow from it,
 * and the mover that puts every block, raw or snappy-compressed, at its final
 * offset.  Implemented by lsbm_amd/liblsbm_crc32c.so with the conventions of
 * include/lsbm_block.h: extern "C", device pointers and an explicit stream
 * (`void*` hipStream_t), calls only enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   table/table_builder.cc:176-206  TableBuilder::WriteBlock: the 12.5 % rule
 *                                   -> lsbm_block_pack_plan_dev
 *   table/table_builder.cc:237-255  WriteRawBlock: file->Append(block_contents),
 *                                   offset += size + kBlockTrailerSize
 *                                   -> lsbm_block_pack_plan_dev, lsbm_block_pack_dev
 *   table/format.cc:66-148          ReadBlock's switch on the type byte: the
 *                                   raw blocks of a batch are moved by
 *                                   lsbm_block_pack_dev (gap 0), the snappy
 *                                   ones by lsbm_snappy_uncompress_dev
 *
 * Handles are {offset, size} pairs of uint64, as everywhere in the block calls.
 * Trailers are not written here: lsbm_sst_seal_dev takes the types.
 *
 * No byte outside the two source images is read and no byte outside a block's
 * destination range is written.  Outputs must not alias inputs: where pointers
 * and sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_TABLE_PACK_H_
#define LSBM_TABLE_PACK_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block_build.h" /* LSBM_BUILD_*, LSBM_* status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_PACK_MAX_BLOCKS (1ull << 31)

/* Per-block status of a batched ReadBlock built from these calls
 * (lsbm_amd.sstable.read_blocks), in the order ReadBlock checks:
 *   LSBM_READ_TRUNCATED       the handle plus its trailer is not inside the
 *                             image (Corruption("truncated block read"))
 *   LSBM_READ_BAD_CHECKSUM    Corruption("block checksum mismatch")
 *   LSBM_READ_BAD_COMPRESSED  GetUncompressedLength or RawUncompress failed
 *                             (Corruption("corrupted compressed block contents"))
 *   LSBM_READ_BAD_TYPE        Corruption("bad block type")
 * and where the reference has no verdict:
 *   LSBM_READ_TOO_LARGE       the batch's snappy preambles ask for more than
 *                             the caller's limit: a compressed block whose
 *                             preamble alone passes the limit, and of the
 *                             others every block at which the running sum of
 *                             the preamble lengths passes it.  Nothing is
 *                             allocated for them (the reference would allocate
 *                             whatever one preamble says, up to 4 GiB). */
#define LSBM_READ_OK 0u
#define LSBM_READ_TRUNCATED 1u
#define LSBM_READ_BAD_CHECKSUM 2u
#define LSBM_READ_BAD_COMPRESSED 3u
#define LSBM_READ_BAD_TYPE 4u
#define LSBM_READ_TOO_LARGE 5u

/* Device scratch either call below needs for n_blocks blocks (bytes; the
 * caller allocates, 8-byte aligned; contents are the call's own). */
uint64_t lsbm_block_pack_scratch_bytes(uint64_t n_blocks);

/* WriteBlock's rule and the layout it leads to.  Per block
 *   type[i]   = d_comp_len[i] != UINT64_MAX
 *               && d_comp_len[i] < d_raw_len[i] - d_raw_len[i] / 8   ? 1 : 0
 *               (unsigned arithmetic as the reference's size_t; a raw length of
 *               0 keeps nothing; UINT64_MAX marks a block that could not be
 *               compressed, port::Snappy_Compress returning false)
 *   size[i]   = type[i] ? d_comp_len[i] : d_raw_len[i]
 *   offset[i] = first_offset + sum over j < i of (size[j] + gap)
 * gap is kBlockTrailerSize (5) for a file and 0 for a plain contents image.
 * Sums wrap at 2^64.  d_comp_len == NULL: every block stays raw.
 * Outputs: d_types[n_blocks], d_handles[2 n_blocks] = {offset, size},
 * d_end[0] = the offset after the last block's gap (first_offset for
 * n_blocks == 0, which is valid). */
int lsbm_block_pack_plan_dev(const uint64_t* d_raw_len, const uint64_t* d_comp_len, uint64_t n_blocks,
                             uint64_t first_offset, uint64_t gap, uint8_t* d_types, uint64_t* d_handles,
                             uint64_t* d_end, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Moves, for every block i, d_handles[2i+1] bytes to d_out + d_handles[2i]:
 * from d_raw + d_raw_handles[2i] when d_types[i] == 0 (of d_raw_handles only
 * the offsets are read), from d_comp + d_comp_offsets[i] when it is 1.
 * Per block, d_status[i]:
 *   LSBM_BUILD_NO_ROOM    the destination range plus gap is not inside
 *                         [0, out_size)
 *   LSBM_BUILD_BAD_INPUT  the source range is not inside its image
 *                         (raw_size / comp_size); the type byte is neither 0
 *                         nor 1; the offsets of its type were not given (NULL)
 * A block in error stores nothing and does not affect the others; with both
 * findings it reports BAD_INPUT.  A size of 0 moves nothing and is OK.
 * Destination ranges are expected not to overlap each other (as
 * lsbm_block_pack_plan_dev lays them out); where they do, the bytes they share
 * are unspecified.  Source and destination phases are unrelated: the stores
 * are aligned 16-byte ones whatever the two are. */
int lsbm_block_pack_dev(const uint8_t* d_raw, uint64_t raw_size, const uint64_t* d_raw_handles,
                        const uint8_t* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets,
                        const uint8_t* d_types, const uint64_t* d_handles, uint64_t n_blocks, uint64_t gap,
                        uint8_t* d_out, uint64_t out_size, uint32_t* d_status, void* d_scratch,
                        uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_TABLE_PACK_H_ */
