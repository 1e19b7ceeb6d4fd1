// bam_host.cpp -- BGZF and BAM on the host (SAMv1 sections 4.1, 4.2): see bam_host.h.
#include "bam_host.h"
#include <zlib.h>
#include <cstdlib>
#include <cstring>

namespace ckm {
namespace bam {
namespace {

inline uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

struct Block { uint64_t comp_off, file_off; uint32_t comp_len, isize, crc; uint64_t out_off; };

// raw deflate of one block into out[0, isize); "" or the reason
std::string inflate_block(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t isize, uint32_t crc) {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) return "inflateInit2 failed";
  uint8_t dummy = 0;
  z.next_in = const_cast<uint8_t *>(in); z.avail_in = n;
  z.next_out = isize ? out : &dummy; z.avail_out = isize ? isize : 1;
  const int rc = inflate(&z, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && z.total_out == isize;
  inflateEnd(&z);
  if (!ok) return "inflate failed";
  if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out, isize) != crc) return "CRC mismatch";
  return "";
}

}  // namespace

uint64_t batch_budget(uint64_t asked) {
  return std::min<uint64_t>(ckm::batch_budget(asked, "CKM_COVERAGE_BATCH_MB", 256), (uint64_t)2 << 30);
}

void Reader::refuse(const std::string &what) const { throw Error(CKM_EINVAL, path_ + ": " + what); }
void Reader::refuse_record(uint64_t ordinal, const std::string &what) const { throw Error(CKM_EINVAL, path_ + ": record " + std::to_string(ordinal) + ": " + what); }

Reader::~Reader() { if (fp_) fclose(fp_); }

void Reader::compact() {
  if (!cur_) return;
  if (len_ > cur_) memmove(buf_.data(), buf_.data() + cur_, len_ - cur_);
  len_ -= cur_; cur_ = 0;
}

bool Reader::more(uint64_t want) {
  if (eof_) return false;
  const WallClock t0;
  std::vector<Block> blocks;
  comp_.clear();
  uint64_t got = 0;
  while (got < want || blocks.empty()) {
    uint8_t h[12];
    const size_t n = fread(h, 1, 12, fp_);
    if (n == 0) { eof_ = true; break; }
    const std::string at = "BGZF block at byte " + std::to_string(file_off_);
    if (n < 12) refuse("truncated " + at);
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) refuse("bad magic in the " + at);
    const uint32_t xlen = ld16(h + 10);
    uint8_t extra[65536];
    if (fread(extra, 1, xlen, fp_) != xlen) refuse("truncated " + at);
    int64_t bsize = -1;
    for (uint32_t p = 0; p + 4 <= xlen;) {
      const uint32_t slen = ld16(extra + p + 2);
      if (extra[p] == 'B' && extra[p + 1] == 'C' && slen == 2 && p + 6 <= xlen) { bsize = ld16(extra + p + 4); break; }
      p += 4 + slen;
    }
    if (bsize < 0) refuse("no BC field in the " + at);
    const int64_t rest = bsize + 1 - 12 - (int64_t)xlen;
    if (rest < 8) refuse("bad BSIZE in the " + at);
    const size_t c0 = comp_.size();
    comp_.resize(c0 + (size_t)rest);
    if (fread(comp_.data() + c0, 1, (size_t)rest, fp_) != (size_t)rest) refuse("truncated " + at);
    const uint8_t *tail = comp_.data() + c0 + rest - 8;
    const uint32_t isize = ld32(tail + 4);
    if (isize > 65536) refuse("ISIZE above 64 KB in the " + at);
    blocks.push_back({c0, file_off_, (uint32_t)(rest - 8), isize, ld32(tail), len_ + got});
    got += isize; file_off_ += (uint64_t)bsize + 1; ++nblocks_;
  }
  timing.ms_read += t0.ms();
  if (blocks.empty()) return false;
  const WallClock t1;
  if (buf_.size() < len_ + got) buf_.resize(len_ + got + (got >> 3));
  auto work = [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const Block &b = blocks[k];
      const std::string why = inflate_block(comp_.data() + b.comp_off, b.comp_len, buf_.data() + b.out_off, b.isize, b.crc);
      if (!why.empty()) refuse(why + " in the BGZF block at byte " + std::to_string(b.file_off));
    }
  };
  if (pool_) pool_->run(blocks.size(), 16, work); else work(0, blocks.size());
  len_ += got; inflated_ += got;
  timing.ms_inflate += t1.ms();
  return true;
}

Reader::Reader(const std::string &path, HostPool *pool) : path_(path), pool_(pool) {
  fp_ = fopen(path.c_str(), "rb");
  if (!fp_) throw Error(CKM_EIO, "cannot open " + path);
  // the header may span blocks: parse, and on running out of bytes fetch more and parse again
  for (;;) {
    const bool grew = more(1 << 16);
    const uint8_t *d = buf_.data();
    uint64_t p = 0;
    bool shortage = false;
    auto need = [&](uint64_t n) { if (p + n > len_) shortage = true; return !shortage; };
    names_.clear(); lengths_.clear();
    do {
      if (!need(12)) break;
      if (memcmp(d, "BAM\1", 4) != 0) refuse("bad magic: not a BAM file");
      const int32_t l_text = (int32_t)ld32(d + 4);
      if (l_text < 0) refuse("negative l_text in the header");
      p = 8 + (uint64_t)l_text;
      if (!need(4)) break;
      const int32_t n_ref = (int32_t)ld32(d + p);
      if (n_ref < 0) refuse("n_ref out of range in the header");
      p += 4;
      for (int32_t r = 0; r < n_ref; ++r) {
        if (!need(4)) break;
        const int32_t l_name = (int32_t)ld32(d + p);
        if (l_name < 1) refuse("reference " + std::to_string(r) + " has no name");
        if (!need(8 + (uint64_t)l_name)) break;
        names_.emplace_back(reinterpret_cast<const char *>(d + p + 4), strnlen(reinterpret_cast<const char *>(d + p + 4), (size_t)l_name));
        lengths_.push_back((int32_t)ld32(d + p + 4 + l_name));
        p += 8 + (uint64_t)l_name;
      }
    } while (false);
    if (!shortage) { cur_ = p; header_bytes_ = p; return; }
    if (!grew) refuse(len_ ? "truncated header" : "bad magic: not a BAM file");
  }
}

bool Reader::next(uint64_t budget, Batch &b) {
  b.offsets.clear(); b.bytes = 0; b.data = nullptr; b.first_ordinal = ordinal_;
  if (!budget) budget = 1;
  if (len_ - cur_ < budget && !eof_) { compact(); more(budget - len_ + (1 << 16)); }      // (slack: the record that straddles the budget)
  const int64_t n_ref = (int64_t)names_.size();
  for (;;) {
    const WallClock t0;
    const uint8_t *d = buf_.data() + cur_;
    const uint64_t n = len_ - cur_;
    uint64_t p = 0;
    b.offsets.clear();
    while (p < budget && p + 4 <= n) {
      const uint64_t ord = ordinal_ + b.offsets.size();
      const int64_t bs = (int32_t)ld32(d + p);
      if (bs < 32) refuse_record(ord, "block_size " + std::to_string(bs) + " is shorter than the fixed part of a record");
      if (p + 4 + (uint64_t)bs > n) break;
      const uint8_t *r = d + p;
      const int64_t ref = (int32_t)ld32(r + 4), l_seq = (int32_t)ld32(r + 20);
      const uint64_t l_name = r[12], n_cigar = ld16(r + 16);
      if (ref < -1 || ref >= n_ref) refuse_record(ord, "refID " + std::to_string(ref) + " out of range");
      if (l_seq < 0) refuse_record(ord, "negative l_seq");
      if (32 + l_name + 4 * n_cigar + (uint64_t)(l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)bs) refuse_record(ord, "the fields run past block_size");
      if (n_cigar == 2 && l_seq > 0) {
        const uint32_t c0 = ld32(r + 36 + l_name), c1 = ld32(r + 40 + l_name);
        if ((c0 & 15) == 4 && (int64_t)(c0 >> 4) == l_seq && (c1 & 15) == 3)
          refuse_record(ord, "the CIGAR is the placeholder of a long CIGAR (real CIGAR in a CG tag): not supported");
      }
      b.offsets.push_back((uint32_t)p);
      p += 4 + (uint64_t)bs;
    }
    timing.ms_offsets += t0.ms();
    if (!b.offsets.empty() && (p >= budget || eof_)) {
      if (eof_ && p < budget && p != n) {
        // the file ended inside a record
        refuse_record(ordinal_ + b.offsets.size(), "the record runs past the end of the file");
      }
      b.data = d; b.bytes = p; cur_ += p; ordinal_ += b.offsets.size();
      return true;
    }
    if (eof_) {
      if (n) refuse_record(ordinal_, "the record runs past the end of the file");
      return false;
    }
    compact();
    more(1 << 16);
  }
}

}  // namespace bam
}  // namespace ckm
