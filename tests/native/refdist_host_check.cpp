// refdist_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the reference-distribution pass (the scaffold join and the argument
// checks of refdist_dev.h, ckm_refdist_check, ckm_refdist_coding over the GFF parsing of ckm_seq_genes_read) built with
// -fsanitize=address,undefined on the CPU and fed the files named on the command line.
//   <fasta> <gff> <seq id> <sep_len>    prints "scaffold=<L>" and the scaffold, the codes of a list of argument checks, then
//                                       "rc=<code> total=<n>" and, for rc=0, the coding bases of the windows [7 k, 7 k + 1 + 13 (k % 9))
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "nucstats_host.h"
#include "refdist_dev.h"

namespace ckm { static std::string g_last; void set_last_error(const std::string &m) { g_last = m; } }

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s <fasta> <gff> <seq id> <sep_len>\n", argv[0]); return 2; }
  ckm_nucseq *b = nullptr;
  const char *paths[1] = {argv[1]};
  if (ckm_nucseq_read(paths, 1, &b)) { printf("rc=-100 %s\n", ckm::g_last.c_str()); return 0; }
  const uint32_t sep = (uint32_t)strtoul(argv[4], nullptr, 10), nseq = (uint32_t)b->seq_off.size();
  const uint64_t L = ckm::rd::scaffold_len(b->seq_bytes.data(), nseq, sep);
  std::vector<uint8_t> scaf;
  ckm::rd::join_scaffold(b->text.data(), b->seq_off.data(), b->seq_bytes.data(), nseq, sep, scaf);
  printf("scaffold=%" PRIu64 " buffer=%zu\n%.*s\n", L, scaf.size(), (int)L, (const char *)scaf.data());
  // the argument checks: fine, a window ending at L, one past it, a negative start, a size of 0, a bad block, a bad stat, no windows
  const int64_t W = (int64_t)L;
  const int64_t st[6] = {0, W > 0 ? W - 1 : 0, 1, -1, 0, W}, sz[6] = {W > 0 ? W : 1, 1, W, 1, 0, 1};
  printf("check=");
  for (int k = 0; k < 6; ++k) printf("%d ", ckm_refdist_check(0, sep, 0, L, st + k, sz + k, 1));
  printf("%d %d %d %d\n", ckm_refdist_check(2, sep, 15, L, st, sz, 0), ckm_refdist_check(3, sep, 16, L, st, sz, 0), ckm_refdist_check(1, sep, 17, L, nullptr, nullptr, 0),
         ckm_refdist_check(1, sep, 16, L, nullptr, nullptr, 1));
  std::vector<int64_t> starts, sizes;
  for (int64_t k = 0; 7 * k < W + 20; ++k) { starts.push_back(7 * k); sizes.push_back(1 + 13 * (k % 9)); }
  std::vector<int64_t> coding(starts.size() + 1, 0);
  int64_t total = -1;
  const int rc = ckm_refdist_coding(argv[2], argv[3], starts.data(), sizes.data(), starts.size(), coding.data(), &total);
  printf("rc=%d total=%" PRId64 " windows=%zu\n", rc, total, starts.size());
  if (rc == 0) { for (size_t x = 0; x < starts.size(); ++x) printf("%" PRId64 " ", coding[x]); printf("\n"); }
  else printf("error: %s\n", ckm::g_last.c_str());
  ckm_nucseq_free(b);
  return 0;
}
