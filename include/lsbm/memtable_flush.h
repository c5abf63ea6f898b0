// include/lsbm/memtable_flush.h -- C++ host API for lsbm's memtable flush:
// what DBImpl::RecoverLogFile and WriteLevel0Table (lsbm/db_impl.cc:433-540)
// do between the log's records and the Level-0 table file, over host buffers.
//
// Mirrors, for all records of one memtable at once:
//   WriteBatchInternal::InsertInto per record (common/write_batch.cc:128-134),
//   MemTable::Add (common/memtable.cc:83-107), the skiplist's order and
//   BuildTable's TableBuilder loop (lsbm/builder.cc:36-48)   -> BuildLevel0
// Sits on top of the C ABI (include/lsbm_memtable.h, lsbm_merge.h,
// lsbm_block_build.h, lsbm_bloom.h, lsbm_crc32c.h): the records go to the
// device in one staging copy and are walked, sorted and built into the table
// there; the table bytes come back.  No HIP types in this header.
#ifndef LSBM_MEMTABLE_FLUSH_H_
#define LSBM_MEMTABLE_FLUSH_H_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "lsbm/status.h"

namespace lsbm {

struct Level0Options {
  uint64_t block_size = 4096;           // Options::block_size
  uint32_t block_restart_interval = 16; // Options::block_restart_interval
  int bits_per_key = -1;                // >= 0: InternalFilterPolicy over NewBloomFilterPolicy(bits_per_key)
  bool paranoid_checks = false;         // true: the first record in error ends the call with its Status
};

// records: the log's logical records as log::ReadLog returns them, each one
// WriteBatch::rep_; all of them are one memtable.  On OK:
//   *file           the kNoCompression table file of the memtable's iteration
//                   under the internal-key comparator; empty when the memtable
//                   has no entry (BuildTable writes no file)
//   *smallest, *largest  the first and the last internal key (FileMetaData)
//   *max_sequence   the largest Sequence + Count - 1 over the records of at
//                   least 12 bytes (0 without one)
//   *record_status  LSBM_WB_* per record (include/lsbm_memtable.h).  Without
//                   paranoid_checks a record in error contributes the entries
//                   before its error, as InsertInto has inserted them.
// With paranoid_checks the first record whose status is not LSBM_WB_OK returns
// Corruption with the reference's message.  A device error returns a non-OK
// Status; *file, *smallest and *largest are then untouched.
Status BuildLevel0(int device, const std::vector<std::string>& records, const Level0Options& options,
                   std::string* file, std::string* smallest, std::string* largest, uint64_t* max_sequence,
                   std::vector<uint32_t>* record_status);

}  // namespace lsbm

#endif  // LSBM_MEMTABLE_FLUSH_H_
