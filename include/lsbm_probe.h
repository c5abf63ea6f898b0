/*
 * lsbm_probe.h -- C ABI of the MI355X (gfx950) probe plan of LSbM's buffered
 * Get: which sorted tables of the compaction and warm-up buffers each query
 * reads, and in which order.  Implemented by lsbm_amd/liblsbm_crc32c.so with
 * the conventions of include/lsbm_get.h: extern "C", device pointers and an
 * explicit stream (`void*` hipStream_t), calls only enqueue, LSBM_* status
 * codes, never throws.
 *
 * Reference interface replaced (lsbm = tengdj/lsbm):
 *   lsbm/version_set.cc:349-623   Version::Get's walk over levels_[level][type]
 *                                 under covered_by_del, covered_by_ins,
 *                                 covered_by_head and checkwb
 *                                             -> lsbm_probe_plan_dev,
 *                                                lsbm_probe_emit_dev
 *
 * A *slot* is one sorted table the walk can reach, in the fixed order in which
 * Version::Get can reach it: Level 0's deletion files (one slot each, newest
 * first) and its insertion table, then per level 1..3 the warm-up tables (WB),
 * the head deletion table (DEL), the head of the compaction buffer (HEAD), the
 * rest of the compaction buffer (REST) and the head insertion table (INS).
 * Which tables are slots (the use lengths' cut of the walks) is the caller's
 * layout, lsbm_amd/buffered.py; every query of a level sees the same slots.
 *
 * d_slot_info[s] = kind | level << 8.  The slots are sorted by (level, kind);
 * a level holds at most one DEL, one HEAD and one INS slot; level-0 slots have
 * the kind LSBM_SLOT_LEVEL0 and no other level does.
 *
 * d_cand is slot-major: d_cand[s * n_queries + q] is what slot s offers query
 * q, after FindFile, the index block's Seek and the filter test:
 *   LSBM_CAND_NONE   no file offered
 *   LSBM_CAND_MISS   the Seek is not valid (and has no error), or the filter says no
 *   LSBM_CAND_MAY    the Seek is valid and the filter passes, or there is no filter
 *   LSBM_CAND_ERR    the Seek ended in an error
 *
 * Per query and level L >= 1 (u = d_use_len[L], user key k):
 *   checkwb        = d_wb_enabled[L] != 0 && k > cursor key L          (:418-421)
 *   covered_by_del = u == 0 && cand[DEL] != NONE                       (:438-440)
 *   if covered_by_del && cand[DEL] == MAY:  the WB slots if checkwb; DEL
 *   if cand[INS] == MAY:                                               (:515-517)
 *     if !covered_by_del:
 *       head_ok = u > 0 && a HEAD slot exists && cand[HEAD] == MAY            (:526)
 *       if (u == 0 || head_ok) && checkwb:  the WB slots
 *       if head_ok:                         HEAD
 *     the REST slots; INS
 * DEL, HEAD and INS are gates: ContainKey is false on an error, so an ERR
 * there reads nothing.  A WB, REST or level-0 slot is a probe when its
 * candidate is MAY (a read) or ERR (the round then returns the error); NONE and
 * MISS are no probe.  Level-0 slots are always walked.  A query's probes are
 * the slots so chosen, in slot order.  d_wb_enabled[L] is the caller's
 * `buffered_merge && L > 1 && use_len[L-1] > 0`.
 *
 * The two-call pattern of the library: lsbm_probe_plan_dev writes d_count[q];
 * the caller's exclusive prefix sum is d_probe_first (n_queries + 1 slots);
 * lsbm_probe_emit_dev writes d_probe_slot[d_probe_first[q] + j], j < count[q].
 *
 * Every call has one status word, d_status[0]: LSBM_MERGE_OK; or
 * LSBM_MERGE_BAD_INPUT where a candidate code is above LSBM_CAND_ERR, a slot's
 * level is above 3 or its kind unknown, the slots are not sorted by (level,
 * kind), a level has two DEL, HEAD or INS slots, a cursor offset decreases or
 * passes its buffer, a lookup key offset decreases, passes its buffer or names
 * a key under 8 bytes, or (emit) d_probe_first does not step by the counts; or
 * (emit) LSBM_MERGE_NO_ROOM where d_probe_first[n_queries] > probe_cap.  On
 * either nothing is written but the status word.  No byte outside a stated
 * size is read or written.  Outputs must not alias inputs: where pointers and
 * sizes show an overlap the call returns LSBM_ERR_INVALID.
 */
#ifndef LSBM_PROBE_H_
#define LSBM_PROBE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsbm_block.h"       /* LSBM_* status codes */
#include "lsbm_block_build.h" /* LSBM_MERGE_OK, LSBM_MERGE_NO_ROOM, LSBM_MERGE_BAD_INPUT */

#ifdef __cplusplus
extern "C" {
#endif

#define LSBM_PROBE_LEVELS 4u /* config::kNumLevels: the entries of d_use_len, d_wb_enabled, the cursor keys */

/* slot kinds, in the order of a level's slots */
#define LSBM_SLOT_LEVEL0 0u
#define LSBM_SLOT_WB 1u
#define LSBM_SLOT_DEL 2u
#define LSBM_SLOT_HEAD 3u
#define LSBM_SLOT_REST 4u
#define LSBM_SLOT_INS 5u

/* candidate codes */
#define LSBM_CAND_NONE 0u
#define LSBM_CAND_MISS 1u
#define LSBM_CAND_MAY 2u
#define LSBM_CAND_ERR 3u

/* d_count[q] = the number of probes of query q.  The lookup keys are those of
 * lsbm_lookup_keys_dev (user key || 8-byte tag); cursor key L is
 * d_cursor_keys[d_cursor_offsets[L], d_cursor_offsets[L+1]) (LSBM_PROBE_LEVELS
 * + 1 offsets), a user key.  One lane per query. */
int lsbm_probe_plan_dev(const uint8_t* d_cand, uint64_t n_slots, const uint32_t* d_slot_info,
                        const uint32_t* d_use_len, const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys,
                        uint64_t cursor_keys_size, const uint64_t* d_cursor_offsets, const uint8_t* d_keys,
                        uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_queries, uint32_t* d_count,
                        uint32_t* d_status, void* stream);

/* d_probe_slot[d_probe_first[q] + j] = the slot of query q's j-th probe.  The
 * inputs are those of the plan call, unchanged. */
int lsbm_probe_emit_dev(const uint8_t* d_cand, uint64_t n_slots, const uint32_t* d_slot_info,
                        const uint32_t* d_use_len, const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys,
                        uint64_t cursor_keys_size, const uint64_t* d_cursor_offsets, const uint8_t* d_keys,
                        uint64_t keys_size, const uint64_t* d_key_offsets, uint64_t n_queries,
                        const uint64_t* d_probe_first, uint32_t* d_probe_slot, uint64_t probe_cap,
                        uint32_t* d_status, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* LSBM_PROBE_H_ */
