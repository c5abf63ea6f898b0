/*
 * lsbm_memtable_cut.h -- C ABI of the MI355X (gfx950) memtable switch: what
 * MemTable::ApproximateMemoryUsage() returns after every record of a log or
 * every group of a write queue, and with it where DBImpl::RecoverLogFile and
 * DBImpl::MakeRoomForWrite end one memtable and begin the next.  Implemented
 * by lsbm_amd/liblsbm_crc32c.so with the conventions of include/lsbm_memtable.h:
 * extern "C", device pointers and an explicit stream (`void*` hipStream_t),
 * calls only enqueue, LSBM_* status codes, never throws.
 *
 * Reference interfaces replaced (lsbm = tengdj/lsbm):
 *   util/random.h                  Random(0xdeadbeef)::Next
 *   common/skiplist.h:240-250      SkipList::RandomHeight (kMaxHeight 12,
 *                                  kBranching 4)
 *                                  -> lsbm_skiplist_heights_dev
 *   util/arena.cc                  Arena::Allocate, AllocateAligned,
 *                                  AllocateFallback, AllocateNewBlock, MemoryUsage
 *   common/memtable.cc:83-107      MemTable::Add's encoded length
 *   common/skiplist.h:180-190      NewNode: 8 + 8 height bytes, aligned
 *   lsbm/db_impl.cc:438-473        RecoverLogFile: a new memtable when there is
 *                                  none, the test after InsertInto
 *   lsbm/db_impl.cc:1469-1505      MakeRoomForWrite: the test before the group
 *                                  -> lsbm_memtable_cut_dev
 *
 * The model.  An entry with internal key length ikl (user key + 8) and value
 * length vl (0 for a deletion) costs Allocate(L), L = VarintLength(ikl) + ikl
 * + VarintLength(vl) + vl, and AllocateAligned(8 + 8 height), where a
 * memtable's j-th insert has the j-th height of the generator's stream from
 * 0xdeadbeef & 0x7fffffff.  The arena is {remaining, n_blocks, blocks_memory}
 * over 4,096-byte blocks, a request above 1,024 bytes that does not fit gets a
 * block of its own, and usage = blocks_memory + 8 * (the least power of two >=
 * n_blocks).  A fresh memtable (its head node allocated) reports 4,104.
 */
#ifndef LSBM_MEMTABLE_CUT_H_
#define LSBM_MEMTABLE_CUT_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_MEMCUT_RECOVER 0u /* RecoverLogFile */
#define LSBM_MEMCUT_WRITE 1u   /* MakeRoomForWrite */

/* the generator's state in a new memtable, and the usage a new memtable reports */
#define LSBM_SKIPLIST_SEED 0x5eadbeefull
#define LSBM_MEMTABLE_FRESH_USAGE 4104ull

/* Device scratch (bytes; the caller allocates, 8-byte aligned, contents are
 * the call's own). */
uint64_t lsbm_skiplist_heights_scratch_bytes(uint64_t n);
uint64_t lsbm_memtable_cut_scratch_bytes(uint64_t n_entries, uint64_t n_records);

/* RandomHeight() of n consecutive inserts from generator state rnd_in
 * (0 < rnd_in < 2^31 - 1, else LSBM_ERR_INVALID; n <= 2^31):
 *   d_heights[n]   1..12
 *   d_rnd_out[0]   the state after them (rnd_in for n == 0) */
int lsbm_skiplist_heights_dev(uint64_t rnd_in, uint64_t n, uint8_t* d_heights, uint64_t* d_rnd_out, void* d_scratch,
                              uint64_t scratch_bytes, void* stream);

/* The accounting of n_records records, record i owning entries
 * [d_entry_base[i], d_entry_base[i+1]).
 *   d_key_offsets[n_entries + 1]  key e is d_key_offsets[e+1] - d_key_offsets[e]
 *                                 bytes; key bytes are never read and only the
 *                                 differences matter
 *   key_extra                     8: the offsets delimit user keys
 *                                 (lsbm_write_sizes_dev's input); 0: internal
 *                                 keys (lsbm_wb_decode_dev's output)
 *   d_values[2 n_entries]         {offset, length}; the offset is not read
 *   d_types[n_entries] or NULL    1 a value, 0 a deletion (its length is not
 *                                 read); NULL: the length is what counts (a
 *                                 deletion of lsbm_wb_decode_dev has 0)
 *   d_rec_status[n_records] or NULL   LSBM_WB_* of lsbm_wb_decode_dev.  RECOVER
 *                                 skips a record that is LSBM_WB_TOO_SMALL,
 *                                 _BAD_INPUT or _NO_ROOM: it creates nothing
 *                                 and tests nothing.  WRITE does not read it.
 *   d_state_in[6] or NULL         {have_mem, remaining, n_blocks, blocks_memory,
 *                                 rnd, entries_in_mem}: a prior call's
 *                                 d_state_out.  NULL: no memtable.
 * RECOVER: a record creates the memtable if there is none, inserts its
 * entries, and then the memtable ends with it if usage > write_buffer_size.
 * WRITE: before a record, the memtable ends and a fresh one begins if usage >
 * write_buffer_size (a memtable is created if there is none); nothing is
 * tested after the last record, the state carries the usage on.
 *   d_usage[n_records]            ApproximateMemoryUsage() after the record
 *                                 (for the record that ends a memtable, what
 *                                 its test saw).  A skipped record repeats
 *                                 its predecessor's, or has 0 while there is
 *                                 no memtable: before the first one and after
 *                                 one has ended
 *   d_mem_first[mem_cap + 1]      the first record of every memtable that takes
 *                                 a record of this call, then n_records
 *   d_mem_usage[mem_cap]          the usage with which each ended, for the last
 *                                 one (if it has not ended) its current usage
 *   d_counts[2]                   {n_memtables, 1 if the first of them is
 *                                 d_state_in's}
 *   d_state_out[6]                have_mem 0 comes with {0, 0, 0, 0,
 *                                 LSBM_SKIPLIST_SEED, 0}
 *   d_status[0]                   LSBM_MERGE_OK; LSBM_MERGE_NO_ROOM: more
 *                                 memtables than mem_cap; LSBM_MERGE_BAD_INPUT:
 *                                 offsets that decrease, an internal key or
 *                                 value length of 2^32 or more, d_entry_base
 *                                 not rising from 0 to n_entries, a type above
 *                                 1, write_buffer_size below 4,104, or a
 *                                 d_state_in no run produces (have_mem above 1,
 *                                 remaining above 4,096 or not a multiple of 8,
 *                                 have_mem without a block, rnd 0 or >= 2^31 - 1)
 * On either error no other output changes.  An overlap between an output and
 * an input or another output, a mode that is neither, a key_extra that is
 * neither 0 nor 8, or more than 2^31 entries or records: LSBM_ERR_INVALID. */
int lsbm_memtable_cut_dev(const uint64_t* d_key_offsets, uint64_t n_entries, uint64_t key_extra,
                          const uint64_t* d_values, const uint8_t* d_types, const uint64_t* d_entry_base,
                          uint64_t n_records, const uint32_t* d_rec_status, uint32_t mode, uint64_t write_buffer_size,
                          const uint64_t* d_state_in, uint64_t* d_usage, uint64_t* d_mem_first, uint64_t* d_mem_usage,
                          uint64_t mem_cap, uint64_t* d_counts, uint64_t* d_state_out, uint32_t* d_status,
                          void* d_scratch, uint64_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_MEMTABLE_CUT_H_ */
