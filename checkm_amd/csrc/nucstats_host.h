// nucstats_host.h -- the batch object of ckm_nucseq_read (not part of the ABI).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace ckm {
struct NucFile {                       // one FASTA file as readFasta leaves it: ids in first-seen order, the last record's sequence
  std::vector<std::string> ids, seqs;
  int err_code = 0;
  std::string err;
};
}  // namespace ckm

struct ckm_nucseq {
  std::vector<char> text;              // sequences at 16-byte boundaries, zero padded, 64 bytes of slack at the end
  std::vector<uint64_t> seq_off, seq_bytes;
  std::vector<uint32_t> file_first;
  std::vector<std::string> ids;
  std::vector<const char *> id_ptr;
};
