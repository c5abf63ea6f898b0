// block_compression.cc -- include/lsbm/block_compression.h on top of the C
// ABI (include/lsbm_snappy.h).  The blocks go to the device once through the
// device's HostSession (host_session.h: persistent streams and buffers, the
// caller's current device restored after), are (de)compressed there in one
// launch, and only the bytes the host keeps come back: compressed blocks are
// compacted on the device first (lsbm_gather_dev), never their capacity slots.
// WriteBlock's keep-or-not rule and the assembly of the output run on the host.
#include "../../include/lsbm/block_compression.h"

#include <hip/hip_runtime_api.h>
#include <string.h>

#include "../../include/lsbm_crc32c.h"
#include "../../include/lsbm_snappy.h"
#include "host_staging.h"

namespace lsbm {

namespace {

// The most a snappy stream of c bytes can expand to: its largest tag ratio
// is a 3-byte copy emitting 64 bytes (21.3x).  A preamble claiming more
// cannot be met, so RawUncompress fails it; it gets no output window.
constexpr uint64_t kMaxExpansion = 22;

}  // namespace

Status CompressBlocks(int device, const char* raw, const uint64_t* offsets, size_t n,
                      std::string* out, std::vector<uint64_t>* out_offsets,
                      std::vector<uint8_t>* types) {
  if (!offsets || !out || !out_offsets || !types) return Status::InvalidArgument("null pointer");
  out->clear();
  out_offsets->assign(1, 0);
  types->clear();
  if (n == 0) return Status::OK();
  if (!raw) return Status::InvalidArgument("null pointer");
  Status s = check_offsets(offsets, n);
  if (!s.ok()) return s;
  const std::vector<uint64_t> off = rebased(offsets, n);
  const uint64_t total = off[n];
  std::vector<uint64_t> cap(n + 1, 0);  // output slots of MaxCompressedLength bytes
  for (size_t i = 0; i < n; i++) cap[i + 1] = cap[i] + lsbm_snappy_max_compressed_length(off[i + 1] - off[i]);

  Staging st;
  s = st.Open(device);
  if (!s.ok()) return s;
  uint8_t* d_raw = st.buf<uint8_t>(0, total);
  uint64_t* d_off = st.buf<uint64_t>(1, n + 1);
  uint64_t* d_cap = st.buf<uint64_t>(2, n + 1);
  uint8_t* d_comp = st.buf<uint8_t>(3, cap[n]);
  uint64_t* d_len = st.buf<uint64_t>(4, n);
  st.put(d_raw, raw + offsets[0], total);
  st.put(d_off, off.data(), n + 1);
  st.put(d_cap, cap.data(), n + 1);
  if (!st.ok()) return st.status("staging");
  if (lsbm_snappy_compress_dev(d_raw, d_off, n, d_comp, d_cap, d_len, st.stream()) != LSBM_OK)
    return Status::IOError(lsbm_crc32c_last_error());
  std::vector<uint64_t> clen(n);
  st.get(clen.data(), d_len, n);
  if (!st.ok()) return st.status("compress");

  // WriteBlock's rule (table/table_builder.cc:187-188), block by block: only
  // the blocks kept compressed have their bytes gathered and brought back
  types->resize(n);
  std::vector<uint64_t> keep_len(n, 0), dense(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    const uint64_t len = off[i + 1] - off[i];
    const bool keep = clen[i] != ~0ull && clen[i] < len - len / 8;
    (*types)[i] = keep ? kSnappyCompression : kNoCompression;
    keep_len[i] = keep ? clen[i] : 0;
    dense[i + 1] = dense[i] + keep_len[i];
  }
  std::string comp(dense[n], '\0');
  if (dense[n]) {
    uint64_t* d_keep = st.buf<uint64_t>(4, n);  // (d_len is no longer needed)
    uint64_t* d_dense = st.buf<uint64_t>(5, n + 1);
    uint8_t* d_packed = st.buf<uint8_t>(6, dense[n]);
    st.put(d_keep, keep_len.data(), n);
    st.put(d_dense, dense.data(), n + 1);
    if (!st.ok()) return st.status("staging");
    if (lsbm_gather_dev(d_comp, d_cap, d_keep, n, d_packed, d_dense, st.stream()) != LSBM_OK)
      return Status::IOError(lsbm_crc32c_last_error());
    st.get(&comp[0], d_packed, dense[n]);
    if (!st.ok()) return st.status("compress");
  }
  out_offsets->resize(n + 1);
  out->reserve(total);
  for (size_t i = 0; i < n; i++) {
    if ((*types)[i] == kSnappyCompression)
      out->append(comp, dense[i], keep_len[i]);
    else
      out->append(raw + offsets[i], off[i + 1] - off[i]);
    (*out_offsets)[i + 1] = out->size();
  }
  return Status::OK();
}

Status UncompressBlocks(int device, const char* data, const uint64_t* offsets, const uint8_t* types,
                        size_t n, std::string* out, std::vector<uint64_t>* out_offsets,
                        std::vector<uint8_t>* ok) {
  if (!offsets || !types || !out || !out_offsets) return Status::InvalidArgument("null pointer");
  out->clear();
  out_offsets->assign(1, 0);
  if (ok) ok->assign(n, 1);
  if (n == 0) return Status::OK();
  if (!data) return Status::InvalidArgument("null pointer");
  Status s = check_offsets(offsets, n);
  if (!s.ok()) return s;

  // the snappy blocks, packed back to back for one launch
  std::vector<size_t> idx;
  std::vector<uint64_t> coff(1, 0);
  for (size_t i = 0; i < n; i++)
    if (types[i] == kSnappyCompression) {
      idx.push_back(i);
      coff.push_back(coff.back() + (offsets[i + 1] - offsets[i]));
    }
  const size_t m = idx.size();
  std::vector<uint64_t> ulen(m, 0);
  std::vector<uint8_t> len_ok(m, 0), dec_ok(m, 0);
  std::vector<uint64_t> uoff(m + 1, 0);
  std::string dec;
  if (m) {
    std::string packed;
    packed.reserve(coff[m]);
    for (size_t j = 0; j < m; j++) packed.append(data + offsets[idx[j]], offsets[idx[j] + 1] - offsets[idx[j]]);
    Staging st;
    s = st.Open(device);
    if (!s.ok()) return s;
    uint8_t* d_comp = st.buf<uint8_t>(0, coff[m]);
    uint64_t* d_coff = st.buf<uint64_t>(1, m + 1);
    uint64_t* d_ulen = st.buf<uint64_t>(2, m);
    uint8_t* d_ok = st.buf<uint8_t>(3, m);
    st.put(d_comp, packed.data(), coff[m]);
    st.put(d_coff, coff.data(), m + 1);
    if (!st.ok()) return st.status("staging");
    // GetUncompressedLength sizes the output windows
    if (lsbm_snappy_uncompressed_length_dev(d_comp, d_coff, m, d_ulen, d_ok, st.stream()) != LSBM_OK)
      return Status::IOError(lsbm_crc32c_last_error());
    st.get(ulen.data(), d_ulen, m);
    st.get(len_ok.data(), d_ok, m);
    if (!st.ok()) return st.status("uncompressed length");
    for (size_t j = 0; j < m; j++) {
      // a preamble no stream of this length can meet fails now, with no window
      if (len_ok[j] && ulen[j] > kMaxExpansion * (coff[j + 1] - coff[j])) len_ok[j] = 0;
      uoff[j + 1] = uoff[j] + (len_ok[j] ? ulen[j] : 0);
    }
    uint8_t* d_out = st.buf<uint8_t>(4, uoff[m]);
    uint64_t* d_uoff = st.buf<uint64_t>(5, m + 1);
    st.put(d_uoff, uoff.data(), m + 1);
    if (!st.ok()) return st.status("staging");
    if (lsbm_snappy_uncompress_dev(d_comp, d_coff, m, d_out, d_uoff, d_ok, nullptr, st.stream()) != LSBM_OK)
      return Status::IOError(lsbm_crc32c_last_error());
    dec.assign(uoff[m], '\0');
    st.get(dec_ok.data(), d_ok, m);
    st.get(&dec[0], d_out, uoff[m]);
    if (!st.ok()) return st.status("uncompress");
  }

  // assemble in block order; the first failing block names the status
  Status first = Status::OK();
  out_offsets->resize(n + 1);
  for (size_t i = 0, j = 0; i < n; i++) {
    bool good = true;
    if (types[i] == kNoCompression) {
      out->append(data + offsets[i], offsets[i + 1] - offsets[i]);
    } else if (types[i] == kSnappyCompression) {
      good = len_ok[j] && dec_ok[j];
      if (good) out->append(dec, uoff[j], uoff[j + 1] - uoff[j]);
      j++;
      if (!good && first.ok()) first = Status::Corruption("corrupted compressed block contents");
    } else {
      good = false;
      if (first.ok()) first = Status::Corruption("bad block type");
    }
    if (ok) (*ok)[i] = good ? 1 : 0;
    (*out_offsets)[i + 1] = out->size();
  }
  return first;
}

}  // namespace lsbm
