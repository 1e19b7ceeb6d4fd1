// seqwin_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the sequence-window pass (ckm_seq_windows_layout,
// ckm_seq_windows_coding over the GFF parsing of ckm_seq_genes_read) built with -fsanitize=address,undefined on the CPU and fed the
// files named on the command line.
//   <fasta> <gff> <window>    prints "rc=<code> missing=<0|1> windows=<n>" and, for rc=0, the coding bases of every window
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"

namespace ckm { static std::string g_last; void set_last_error(const std::string &m) { g_last = m; } }

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <fasta> <gff> <window>\n", argv[0]); return 2; }
  ckm_nucseq *b = nullptr;
  const char *paths[1] = {argv[1]};
  if (ckm_nucseq_read(paths, 1, &b)) { printf("rc=-100 %s\n", ckm::g_last.c_str()); return 0; }
  ckm_nucseq_view v;
  ckm_nucseq_view_get(b, &v);
  const int64_t w = strtoll(argv[3], nullptr, 10);
  std::vector<int64_t> first(v.nseq + 1, 0);
  int rc = ckm_seq_windows_layout(b, w, first.data());
  if (rc) { printf("rc=%d layout: %s\n", rc, ckm::g_last.c_str()); ckm_nucseq_free(b); return 0; }
  std::vector<int64_t> coding((size_t)first[v.nseq] + 1, 0);
  uint8_t missing[1] = {0};
  const char *gffs[1] = {argv[2]};
  rc = ckm_seq_windows_coding(gffs, b, w, coding.data(), missing);
  printf("rc=%d missing=%d windows=%" PRId64 "\n", rc, (int)missing[0], first[v.nseq]);
  if (rc == 0) { for (int64_t x = 0; x < first[v.nseq]; ++x) printf("%" PRId64 " ", coding[x]); printf("\n"); }
  else printf("error: %s\n", ckm::g_last.c_str());
  ckm_nucseq_free(b);
  return 0;
}
