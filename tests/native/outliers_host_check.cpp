// outliers_host_check.cpp -- TEST INFRASTRUCTURE: the two host readers of the outlier pass (ckm_tetra_profile_read, ckm_seq_genes_read)
// built with -fsanitize=address,undefined on the CPU and fed the files named on the command line.
//   profile <file>            prints "rc=<code> n=<rows>" and, for rc=0, every row's id and the hexadecimal bits of its first and last value
//   genes <fasta> <gff>       prints "rc=<code> missing=<0|1>" and the coding bases of every sequence
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"

namespace ckm { static std::string g_last; void set_last_error(const std::string &m) { g_last = m; } }

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "profile")) {
    ckm_tetra_profile *p = nullptr;
    const int rc = ckm_tetra_profile_read(argv[2], &p);
    ckm_tetra_profile_view v = {0, nullptr, nullptr};
    if (rc == 0) ckm_tetra_profile_view_get(p, &v);
    printf("rc=%d n=%u\n", rc, v.n);
    for (uint32_t i = 0; i < v.n; ++i) {
      uint64_t a, z;
      memcpy(&a, v.sig + (size_t)i * 136, 8); memcpy(&z, v.sig + (size_t)i * 136 + 135, 8);
      printf("%s %016" PRIx64 " %016" PRIx64 "\n", v.ids[i], a, z);
    }
    if (rc) printf("error: %s\n", ckm::g_last.c_str());
    ckm_tetra_profile_free(p);
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "genes")) {
    ckm_nucseq *b = nullptr;
    const char *paths[1] = {argv[2]};
    if (ckm_nucseq_read(paths, 1, &b)) { printf("rc=-100 %s\n", ckm::g_last.c_str()); return 0; }
    ckm_nucseq_view v;
    ckm_nucseq_view_get(b, &v);
    std::vector<int64_t> coding(v.nseq + 1, 0);
    uint8_t missing[1] = {0};
    const char *gffs[1] = {argv[3]};
    const int rc = ckm_seq_genes_read(gffs, b, coding.data(), missing);
    printf("rc=%d missing=%d\n", rc, (int)missing[0]);
    if (rc == 0) for (uint32_t s = 0; s < v.nseq; ++s) printf("%s %" PRId64 "\n", v.seq_ids[s], coding[s]);
    else printf("error: %s\n", ckm::g_last.c_str());
    ckm_nucseq_free(b);
    return 0;
  }
  fprintf(stderr, "usage: %s profile <file> | genes <fasta> <gff>\n", argv[0]);
  return 2;
}
