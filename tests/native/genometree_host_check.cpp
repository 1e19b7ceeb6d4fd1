// genometree_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the genome tree (ckm_gtree_check and ckm_gtree_host in
// gtree_host.cpp; the encoding, the counts, the distances, the joins and the batch cuts of gtree_dev.h) built with
// -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers: N L nreps base model, max_dist as %a, then N * L byte values, then nreps * L columns.
// Prints "check rc=<code>", "counts <sum of compared> <sum of differ>", one line "<tree> <row> <i> <j> <two doubles as %a>" per merge
// row and "rounds <n>"; then, <damaged calls> times, the call with entries overwritten is checked ("damaged rc=<code>") and, where the
// check passes, run as well.  Every array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  uint32_t N = 0, L = 0, nreps = 0, base = 0;
  int32_t model = 0;
  double max_dist = 0;
  std::vector<uint8_t> text;
  std::vector<uint32_t> cols;
  ckm_gtree_args args() const {
    ckm_gtree_args a = {};
    a.nrows = N; a.ncols = L; a.text = text.data(); a.ntext_bytes = text.size(); a.nreps = nreps; a.cols = cols.data(); a.base = base; a.model = model; a.max_dist = max_dist;
    return a;
  }
};

static void walk(const Call &c, uint64_t budget, bool print) {
  const ckm_gtree_args a = c.args();
  const size_t N = a.nrows, T = (size_t)a.base + a.nreps;
  std::vector<uint32_t> cmp(N * N), dif(N * N), ij(T * (N - 1) * 2);
  std::vector<double> dist(N * N), len(T * (N - 1) * 2);
  ckm_gtree_out o = {cmp.data(), dif.data(), dist.data(), ij.data(), len.data()};
  ckm_gtree_info info;
  const int rc = ckm_gtree_host(&a, budget, &o, &info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  uint64_t sc = 0, sd = 0;
  for (size_t k = 0; k < N * N; ++k) { sc += cmp[k]; sd += dif[k]; if (!(dist[k] >= 0.0)) { printf("a distance that was never written\n"); exit(6); } }
  if (print) printf("counts %" PRIu64 " %" PRIu64 "\n", sc, sd);
  for (size_t t = 0; t < T; ++t)
    for (size_t r = 0; r + 1 < N; ++r) {
      const size_t at = (t * (N - 1) + r) * 2;
      if (ij[at] >= N || ij[at + 1] >= N || !(len[at] >= 0.0) || !(len[at + 1] >= 0.0)) { printf("a merge row that was never written\n"); exit(6); }
      if (print) printf("%zu %zu %u %u %a %a\n", t, r, ij[at], ij[at + 1], len[at], len[at + 1]);
    }
  if (print) printf("rounds %" PRIu64 "\n", (uint64_t)info.nrounds);
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  bool ok = fscanf(f, "%u %u %u %u %d %la", &c.N, &c.L, &c.nreps, &c.base, &c.model, &c.max_dist) == 6;
  const uint64_t cap = 1u << 22;
  ok = ok && (uint64_t)c.N * c.L < cap && (uint64_t)c.nreps * c.L < cap;
  if (ok) {
    c.text.resize((size_t)c.N * c.L); c.cols.resize((size_t)c.nreps * c.L);
    for (auto &b : c.text) { unsigned v = 0; ok = ok && fscanf(f, "%u", &v) == 1; b = (uint8_t)v; }
    for (auto &v : c.cols) ok = ok && fscanf(f, "%" SCNu32, &v) == 1;
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_gtree_args a = c.args();
  const int rc = ckm_gtree_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  static const double dists[] = {-1.0, 0.0, 0.5, 3.0, 1e300, 1.0 / 0.0, 0.0 / 0.0};
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 7) {
        case 0: if (!d.text.empty()) d.text[rnd() % d.text.size()] = (uint8_t)rnd(); break;
        case 1: if (!d.cols.empty()) d.cols[rnd() % d.cols.size()] = (uint32_t)(rnd() % 3 ? rnd() % (d.L + 2) : rnd()); break;
        case 2: d.model = (int32_t)(rnd() % 5) - 1; break;
        case 3: d.max_dist = dists[rnd() % 7]; break;
        case 4: d.base = (uint32_t)(rnd() % 3); break;
        case 5: d.N = (uint32_t)(rnd() % 4 ? rnd() % (c.N + 2) : rnd()); break;          // (the text keeps its size: a count that does not match it is refused)
        default: d.L = (uint32_t)(rnd() % 4 ? rnd() % (c.L + 2) : rnd()); break;
      }
    a = d.args();
    const int drc = ckm_gtree_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
