"""lsbm_amd -- MI355X-native batched CRC-32C engine for lsbm's block checksums.

  lsbm_amd.crc32c   util/crc32c.h mirror (Value / Extend / Mask / Unmask)
  lsbm_amd.engine   device-resident and host-staged batches (GPU)
  lsbm_amd.table    SSTable block trailers: batched WriteRawBlock / ReadBlock verify
  lsbm_amd.log      WAL / MANIFEST record CRCs: batched log::Writer seal / log::Reader check; the batched
                    log::Reader itself: block walk, ReadRecord with every Reporter call (read_records)
  lsbm_amd.bloom    SSTable bloom filters: batched CreateFilter / KeyMayMatch / filter blocks
  lsbm_amd.snappy   SSTable block compression: batched snappy RawCompress / RawUncompress
  lsbm_amd.block    SSTable block reader: batched Block::Iter scan / decode / Seek, Table::InternalGet
  lsbm_amd.block_build  SSTable block builder: batched flush plan, BlockBuilder Add / Finish, index
                    blocks, whole table files
  lsbm_amd.merge    compaction merge: batched MergingIterator over sorted runs, DoCompactionWork's
                    drop rule and output-file cut, input table images -> output table files
  lsbm_amd.sstable  tables with snappy-compressed blocks: WriteBlock's keep rule and block packing,
                    batched ReadBlock, Get and compaction over either block type, and the one table
                    writer (write_tables / finish_tables) that block_build, merge and memtable write through
  lsbm_amd.memtable memtable flush: batched WriteBatch::Iterate over log records, the memtable's
                    iteration order as a sort, log image -> Level-0 table file (recover: RecoverLogFile
                    over a log in device memory)
  lsbm_amd.db       batched DB::Get: LookupKey, MemTable::Get, FindFile, SaveValue, and the chain over
                    memtables and table files (Version.get)
  lsbm_amd.scan     batched range scans: DBIter's snapshot view of merged entries, Seek / SeekToFirst /
                    SeekToLast / Next / Prev / status for many range queries at once (Version.view)
  lsbm_amd.write    batched DB::Write: WriteBatch::Put / Delete encoding, BuildBatchGroup's rule, the
                    groups' reps and sequence numbers, log::Writer::AddRecord's framing (write_batches)
  lsbm_amd.manifest MANIFEST snapshots: batched VersionEdit::DecodeFrom / EncodeTo, the entries of one
                    long record found in parallel, WriteSnapshot's record from a device-resident file
                    table (snapshot, manifest_image), BasicVersionSet::Recover's loop (recover)
  lsbm_amd.buffered LSbM's buffered Get: Builder::SaveTo's sorted-table lists, the slots Version::Get can reach,
                    the probe plan under covered_by_del / covered_by_ins / covered_by_head / checkwb, and
                    table reads by probe rank (BufferedVersion.get, from_manifest)
  lsbm_amd.rangequery  LSbM's RangeQuery over the buffered tree: the files Version::RangeQuery reads under
                    checkwb / wb_covered / dl_covered / cb_covered, and TableCache::GetRange's Seek and count
                    up to the end key over a range index of the opened files (RangeQuery.query)

The compute lives in lsbm_amd/liblsbm_crc32c.so (hand-written gfx950 HIP
kernels behind the C ABIs in include/lsbm_crc32c.h, include/lsbm_bloom.h, include/lsbm_snappy.h and
include/lsbm_block.h, include/lsbm_block_build.h, include/lsbm_merge.h, include/lsbm_table_pack.h,
include/lsbm_memtable.h, include/lsbm_get.h, include/lsbm_iter.h, include/lsbm_write.h, include/lsbm_log_read.h,
include/lsbm_manifest.h, include/lsbm_probe.h, include/lsbm_range.h).
"""
from ._lib import LIB_PATH, LsbmError, lib  # noqa: F401

__all__ = ["LIB_PATH", "LsbmError", "lib", "crc32c", "engine", "table", "log", "bloom", "snappy",
           "block", "block_build", "merge", "sstable", "memtable", "db", "scan", "write", "manifest", "buffered",
           "rangequery"]
