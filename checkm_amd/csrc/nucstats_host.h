// nucstats_host.h -- the batch object of ckm_nucseq_read and the host helpers its readers share (not part of the ABI).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

namespace ckm {
// the whole file ('.gz' names through zlib); false and a message in err when it cannot be read
bool read_bytes(const char *path, std::string &buf, std::string &err);

// f(0) .. f(n - 1) on up to 16 host threads
template <class F>
inline void for_each_parallel(uint32_t n, F &&f) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const unsigned nt = std::min<unsigned>(std::min<unsigned>(hw, 16u), std::max(1u, n));
  std::atomic<uint32_t> next(0);
  auto work = [&] { for (uint32_t b; (b = next.fetch_add(1)) < n;) f(b); };
  std::vector<std::thread> th;
  for (unsigned k = 1; k < nt; ++k) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
}

struct NucFile {                       // one FASTA file as readFasta leaves it: ids in first-seen order, the last record's sequence
  std::vector<std::string> ids, seqs;
  std::vector<uint64_t> nbytes, ncp;   // read without text (ckm_fasta_ids_read): bytes and code points per id instead of seqs
  int err_code = 0;
  std::string err;
};
}  // namespace ckm

struct ckm_nucseq {
  std::vector<char> text;              // sequences at 16-byte boundaries, zero padded, 64 bytes of slack at the end
  std::vector<uint64_t> seq_off, seq_bytes;
  std::vector<uint64_t> seq_cp;        // code points of every sequence (len(seq) of the Python str), counted once when the batch is read
  std::vector<uint32_t> file_first;
  std::vector<std::string> ids;
  std::vector<const char *> id_ptr;
};

struct ckm_fasta_ids {                 // ckm_fasta_ids_read: what ckm_nucseq keeps, without the text
  std::vector<uint64_t> seq_bytes, seq_cp;
  std::vector<uint32_t> file_first;
  std::vector<std::string> ids;
  std::vector<const char *> id_ptr;
};

namespace ckm {
// first window of every sequence of a batch for windows of w, from b->seq_cp (seqwin_dev.h); CKM_ERANGE beyond 2^31 - 1 windows
void window_layout(const ckm_nucseq *b, uint64_t w, std::vector<uint64_t> &first);
}  // namespace ckm
