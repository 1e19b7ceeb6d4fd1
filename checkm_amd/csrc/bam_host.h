// bam_host.h -- the host reader of `checkm coverage`: BGZF blocks inflated on the host pool, the BAM header, and batches of whole
// records with one offset per record (bam_host.cpp).  Plain C++ and zlib, no device: tests/native/bam_host_check.cpp and
// tests/emu/coverage_emu.cpp build it with g++.  The .bai index is not read.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "host_pool.h"

namespace ckm {
namespace bam {

struct Timing { double ms_read = 0, ms_inflate = 0, ms_offsets = 0; };

// One batch: records [first_ordinal, first_ordinal + offsets.size()) of the file; offsets are relative to `data`, which holds `bytes`
// bytes of whole records.  The pointers stay valid until the next call of Reader::next.
struct Batch {
  const uint8_t *data = nullptr;
  uint64_t bytes = 0, first_ordinal = 0;
  std::vector<uint32_t> offsets;
};

class Reader {
 public:
  Reader(const std::string &path, HostPool *pool);      // opens the file and parses the header; throws Error(CKM_EIO / CKM_EINVAL)
  ~Reader();
  Reader(const Reader &) = delete; Reader &operator=(const Reader &) = delete;
  const std::string &path() const { return path_; }
  const std::vector<std::string> &ref_names() const { return names_; }
  const std::vector<int64_t> &ref_lengths() const { return lengths_; }
  uint64_t header_bytes() const { return header_bytes_; }       // inflated bytes in front of the first record
  uint64_t blocks() const { return nblocks_; }
  uint64_t inflated() const { return inflated_; }
  // The next records: a batch ends at the first record boundary at or beyond `budget` inflated bytes (at least one record).  false at
  // the end of the file.  Every refusal names the file and the record's ordinal.
  bool next(uint64_t budget, Batch &b);
  Timing timing;
 private:
  bool more(uint64_t want);          // appends inflated blocks until `want` more bytes have arrived or the file ends
  void compact();
  [[noreturn]] void refuse(const std::string &what) const;
  [[noreturn]] void refuse_record(uint64_t ordinal, const std::string &what) const;
  std::string path_; HostPool *pool_; FILE *fp_ = nullptr;
  std::vector<std::string> names_; std::vector<int64_t> lengths_;
  std::vector<uint8_t> buf_, comp_; uint64_t cur_ = 0, len_ = 0;
  uint64_t header_bytes_ = 0, nblocks_ = 0, inflated_ = 0, file_off_ = 0, ordinal_ = 0;
  bool eof_ = false;
};

uint64_t batch_budget(uint64_t asked);     // asked, or CKM_COVERAGE_BATCH_MB (default 256) in bytes; at most 2 GB

}  // namespace bam
}  // namespace ckm
