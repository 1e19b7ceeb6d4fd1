// selection_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the marker-set selection (ckm_select_check in select_host.cpp; the
// generator, the draw, the packing and the round cuts of select_dev.h, walked by the host executor of tests/emu/selection_emu.cpp, which
// this file includes) built with -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers: G U S R nkeys ncs nmembers contig_len seed, then comp_lo comp_hi cont_lo cont_hi as %a;
// G genome lengths; G * U + 1 key offsets; the keys; S + 1 marker set offsets; ncs + 1 co-located set offsets; the members.  Prints
// "check rc=<code>", one line "<genome> <replicate> <trueComp> <trueCont> <row sum>" per draw and one line "<genome> <replicate>
// <marker set> <four doubles as %a>" per result, then "rounds <n>"; then, <damaged calls> times, the call with entries overwritten is
// checked ("damaged rc=<code>") and, where the check passes, walked as well.  Every array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "../emu/selection_emu.cpp"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  std::vector<int64_t> genome_len, key;
  std::vector<uint64_t> key_off, ms_off, cs_off;
  std::vector<uint32_t> cs_marker;
  uint32_t U = 0, R = 0;
  int64_t contig_len = 0;
  double f[4] = {0, 0, 0, 0};
  uint64_t seed = 0;
  ckm_select_args args() const {
    ckm_select_args a;
    a.ngenomes = (uint32_t)genome_len.size(); a.genome_len = genome_len.data();
    a.nmarkers = U; a.key_off = key_off.data(); a.key = key.data(); a.nkeys = key.size();
    a.nsets = (uint32_t)ms_off.size() - 1; a.ms_off = ms_off.data(); a.cs_off = cs_off.data(); a.ncs = cs_off.size() - 1;
    a.cs_marker = cs_marker.data(); a.nmembers = cs_marker.size();
    a.nreplicates = R; a.contig_len = contig_len; a.comp_lo = f[0]; a.comp_hi = f[1]; a.cont_lo = f[2]; a.cont_hi = f[3]; a.seed = seed;
    return a;
  }
};

static void walk(const Call &c, uint64_t budget, bool print) {
  const ckm_select_args a = c.args();
  const size_t D = (size_t)a.ngenomes * a.nreplicates;
  size_t nrow = 0;
  for (uint32_t g = 0; g < a.ngenomes; ++g) nrow += (size_t)(a.genome_len[g] / a.contig_len) * a.nreplicates;
  std::vector<double> truth(D * 2), out(D * a.nsets * 4);
  std::vector<uint16_t> rows(nrow);
  uint64_t info[1] = {0};
  const int rc = emu_select_run(&a, budget, truth.data(), out.data(), rows.data(), info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  size_t at = 0;
  for (uint32_t g = 0; g < a.ngenomes; ++g)
    for (uint32_t r = 0; r < a.nreplicates; ++r) {
      const size_t d = (size_t)g * a.nreplicates + r, C = (size_t)(a.genome_len[g] / a.contig_len);
      uint64_t sum = 0;
      for (size_t i = 0; i < C; ++i) sum += rows[at + i];
      at += C;
      if (!(truth[d * 2] >= 0.0) || !(truth[d * 2 + 1] >= 0.0)) { printf("a true value that was never written\n"); exit(6); }
      if (print) printf("%u %u %a %a %" PRIu64 "\n", g, r, truth[d * 2], truth[d * 2 + 1], sum);
      for (uint32_t s = 0; s < a.nsets; ++s) {
        const double *o = &out[(d * a.nsets + s) * 4];
        for (int k = 0; k < 4; ++k)
          if (!(o[k] >= 0.0)) { printf("a result that was never written\n"); exit(6); }
        if (print) printf("%u %u %u %a %a %a %a\n", g, r, s, o[0], o[1], o[2], o[3]);
      }
    }
  if (print) printf("rounds %" PRIu64 "\n", info[0]);
}

template <class T, class Read>
static bool read_n(FILE *f, std::vector<T> &v, size_t n, Read &&read) {
  v.resize(n);
  for (size_t k = 0; k < n; ++k)
    if (!read(f, v[k])) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  unsigned G = 0, S = 0;
  uint64_t nkeys = 0, ncs = 0, nmembers = 0;
  auto u64 = [](FILE *g, uint64_t &x) { return fscanf(g, "%" SCNu64, &x) == 1; };
  auto i64 = [](FILE *g, int64_t &x) { return fscanf(g, "%" SCNd64, &x) == 1; };
  auto u32 = [](FILE *g, uint32_t &x) { return fscanf(g, "%" SCNu32, &x) == 1; };
  bool ok = fscanf(f, "%u %u %u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64 " %la %la %la %la", &G, &c.U, &S, &c.R, &nkeys, &ncs, &nmembers, &c.contig_len,
                   &c.seed, &c.f[0], &c.f[1], &c.f[2], &c.f[3]) == 13;
  const uint64_t cap = 1u << 22;
  ok = ok && G < cap && c.U < cap && S < cap && c.R < cap && nkeys < cap && ncs < cap && nmembers < cap && (uint64_t)G * c.U < cap;
  ok = ok && read_n(f, c.genome_len, G, i64) && read_n(f, c.key_off, (size_t)G * c.U + 1, u64) && read_n(f, c.key, nkeys, i64) && read_n(f, c.ms_off, (size_t)S + 1, u64) &&
       read_n(f, c.cs_off, ncs + 1, u64) && read_n(f, c.cs_marker, nmembers, u32);
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_select_args a = c.args();
  const int rc = ckm_select_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto hit_offsets = [&](std::vector<uint64_t> &t) { t[rnd() % t.size()] = rnd() % 4 == 0 ? rnd() : rnd() % (t.back() + 3); };
  auto hit_values = [&](std::vector<int64_t> &t, uint64_t span) {
    if (!t.empty()) t[rnd() % t.size()] = rnd() % 3 ? (int64_t)(rnd() % span) - 1000 : (int64_t)rnd();
  };
  static const double fractions[] = {-0.25, 0.0, 0.3, 1.0, 1.5, 8.0, 8.5, 1e300};
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 8) {
        case 0: hit_offsets(d.key_off); break;
        case 1: hit_offsets(d.ms_off); break;
        case 2: hit_offsets(d.cs_off); break;
        case 3: if (!d.cs_marker.empty()) d.cs_marker[rnd() % d.cs_marker.size()] = (uint32_t)(rnd() % 3 ? rnd() % (d.U + 1) : rnd()); break;
        case 4: hit_values(d.key, 1ull << 32); break;
        case 5: hit_values(d.genome_len, 1ull << 21); break;          // up to 2^21 bases: with the call's contig length within the contigs a block keeps, or just beyond
        case 6: d.f[rnd() % 4] = fractions[rnd() % 8]; break;
        default: d.contig_len = rnd() % 4 ? (int64_t)(rnd() % 3000) : (int64_t)rnd(); break;
      }
    a = d.args();
    const int drc = ckm_select_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
