// queue_set_check.cpp -- csrc/queue_set.h alone, on the host: the exclusive prefix of the clamped queue lengths and the map from a flat
// item number to (queue, position).  Reads a case file
//   n
//   count[0] cap[0] ... count[n-1] cap[n-1]
//   m
//   k[0] ... k[m-1]
// and prints {"pre": [...], "total": t, "at": [[found, queue, pos], ...]} (queue and pos are -1 where k is no item: the function must
// leave its outputs alone then).  tests/test_queue_set_host.py compiles it with AddressSanitizer and UBSan and holds the output against a
// restatement in Python.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "queue_set.h"

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: queue_set_check <case file>\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned n = 0, m = 0;
  if (fscanf(f, "%u", &n) != 1 || n > 100000) return 2;
  // exactly n counts, n caps and n + 1 prefix entries: the sanitizer sees any access beyond them
  std::vector<uint32_t> count(n), cap(n), pre((size_t)n + 1);
  for (unsigned i = 0; i < n; ++i) if (fscanf(f, "%u %u", &count[i], &cap[i]) != 2) return 2;
  if (fscanf(f, "%u", &m) != 1 || m > 10000000) return 2;
  std::vector<uint32_t> ks(m);
  for (unsigned i = 0; i < m; ++i) if (fscanf(f, "%u", &ks[i]) != 1) return 2;
  fclose(f);
  const uint32_t total = ckm::qs_prefix(count.data(), cap.data(), n, pre.data());
  printf("{\"pre\": [");
  for (unsigned i = 0; i <= n; ++i) printf("%s%u", i ? ", " : "", pre[i]);
  printf("], \"total\": %u, \"at\": [", total);
  for (unsigned i = 0; i < m; ++i) {
    uint32_t q = 0xffffffffu, pos = 0xffffffffu;
    const bool found = ckm::qs_locate(pre.data(), n, ks[i], q, pos);
    printf("%s[%d, %lld, %lld]", i ? ", " : "", found ? 1 : 0, q == 0xffffffffu ? -1ll : (long long)q, pos == 0xffffffffu ? -1ll : (long long)pos);
  }
  printf("]}\n");
  return 0;
}
