// nearid_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the near-identity pass (ckm_nearid_check and ckm_nearid_host in
// nearid_host.cpp; the check, the word arithmetic and the band cuts of nearid_dev.h) built with -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers: n_rows, row_len, row_stride, then the limits [n_rows], then the text [n_rows * row_stride]
// byte by byte.  Prints "check rc=<code>", one line "w <row> <word as hex> ..." per row and "bands <n>"; then, <damaged calls> times, a
// call over the same buffers with fewer rows, another row length, another stride (never more than the buffers hold: the library cannot
// know their extent), limits overwritten (0 among them) and text bytes overwritten is checked ("damaged rc=<code>") and, where the check
// passes, run as well.  Every array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

static void walk(const ckm_nearid_args &a, uint64_t budget, bool print) {
  const size_t W = ((size_t)a.n_rows + 63) / 64;
  std::vector<uint64_t> near((size_t)a.n_rows * W, 0x5555555555555555ull);      // exactly the matrix; a pattern no row of the tests can give
  ckm_nearid_out o = {near.data()};
  ckm_nearid_info info;
  const int rc = ckm_nearid_host(&a, budget, &o, &info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  for (size_t i = 0; i < a.n_rows; ++i) {
    for (size_t j = 0; j <= i; ++j)
      if (near[i * W + j / 64] >> (j % 64) & 1) { printf("a bit at or below the diagonal\n"); exit(6); }
    for (size_t j = a.n_rows; j < W * 64; ++j)
      if (near[i * W + j / 64] >> (j % 64) & 1) { printf("a bit beyond the last row\n"); exit(6); }
    if (print) {
      printf("w %zu", i);
      for (size_t w = 0; w < W; ++w) printf(" %" PRIx64, near[i * W + w]);
      printf("\n");
    }
  }
  if (print) printf("bands %" PRIu64 "\n", (uint64_t)info.nbands);
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t N = 0, L = 0, S = 0;
  const uint64_t cap = 1u << 24;
  bool ok = fscanf(f, "%u %u %u", &N, &L, &S) == 3 && (uint64_t)N * S < cap && N < cap;
  std::vector<uint32_t> limit(ok ? N : 0);
  std::vector<uint8_t> text(ok ? (size_t)N * S : 0);
  for (auto &x : limit) ok = ok && fscanf(f, "%" SCNu32, &x) == 1;
  for (auto &x : text) { unsigned v = 0; ok = ok && fscanf(f, "%u", &v) == 1 && v < 256; x = (uint8_t)v; }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_nearid_args a = {text.data(), N, L, S, limit.data()};
  const int rc = ckm_nearid_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(a, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    std::vector<uint32_t> dl = limit;
    std::vector<uint8_t> dt = text;
    uint32_t dS = S, dL = L, dN = N;
    switch (rnd() % 6) {
      case 0: dS = (uint32_t)(rnd() % (S + 17)); break;                             // any stride, mostly no multiple of 16
      case 1: dS = (uint32_t)(16 * (rnd() % (S / 16 + 1))); break;                  // a multiple of 16 up to the real one, 0 among them
      case 2: dL = (uint32_t)(rnd() % (S + 3)); break;                              // a row length up to just beyond the stride
      case 3: dL = (uint32_t)(rnd() % 18); break;                                   // short rows, 0 among them
      default: break;
    }
    if (rnd() % 4 == 0) dN = (uint32_t)(rnd() % (N + 1));
    while ((uint64_t)dN * dS > text.size()) --dN;                                  // (never more than the buffers hold)
    for (int hits = (int)(rnd() % 4); hits > 0 && !dl.empty(); --hits) dl[rnd() % dl.size()] = (uint32_t)(rnd() % 3 ? rnd() % 4 : rnd());
    for (int hits = (int)(rnd() % 64); hits > 0 && !dt.empty(); --hits) dt[rnd() % dt.size()] = (uint8_t)rnd();
    ckm_nearid_args d = {dt.data(), dN, dL, dS, dl.data()};
    const int drc = ckm_nearid_check(&d);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
