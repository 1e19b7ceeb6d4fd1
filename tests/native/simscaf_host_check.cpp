// simscaf_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the scaffold simulation (ckm_simscaf_check in simscaf_host.cpp; the
// packing, the round cuts and the per-copy step of simscaf_dev.h, walked by the host executor of tests/emu/simscaf_emu.cpp, which this file
// includes) built with -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers: G U S R nsc ncs nmembers nwords; G scaffold counts; G * U + 1 cell offsets; the scaffold
// indices; S + 1 marker set offsets; ncs + 1 co-located set offsets; the members; R test genomes; R contaminants; R + 1 bit offsets; the
// words.  Prints "check rc=<code>", one line "<replicate> <marker set> <four doubles as %a>" per result and "rounds <n>"; then, <damaged
// calls> times, the call with entries overwritten is checked ("damaged rc=<code>") and, where the check passes, walked as well.  Every
// array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "../emu/simscaf_emu.cpp"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  uint32_t U = 0;
  std::vector<uint64_t> sc_off, ms_off, cs_off, bit_off;
  std::vector<uint32_t> nscaf, sc, cs_marker, test, cont, bits;
  ckm_simscaf_args args() const {
    ckm_simscaf_args a;
    a.ngenomes = (uint32_t)nscaf.size(); a.nscaf = nscaf.data(); a.nmarkers = U; a.sc_off = sc_off.data(); a.sc = sc.data(); a.nsc = sc.size();
    a.nsets = (uint32_t)ms_off.size() - 1; a.ms_off = ms_off.data(); a.cs_off = cs_off.data(); a.ncs = cs_off.size() - 1;
    a.cs_marker = cs_marker.data(); a.nmembers = cs_marker.size();
    a.nreplicates = (uint32_t)test.size(); a.test = test.data(); a.cont = cont.data(); a.bit_off = bit_off.data(); a.bits = bits.data(); a.nwords = bits.size();
    return a;
  }
};

static double walk(const Call &c, uint64_t budget, bool print) {
  const ckm_simscaf_args a = c.args();
  std::vector<double> out((size_t)a.nreplicates * a.nsets * 4);
  uint64_t info[1] = {0};
  const int rc = emu_simscaf_run(&a, budget, out.data(), info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  double sum = 0;
  for (uint32_t r = 0; r < a.nreplicates; ++r)
    for (uint32_t s = 0; s < a.nsets; ++s) {
      const double *o = &out[((size_t)r * a.nsets + s) * 4];
      for (int k = 0; k < 4; ++k) {
        if (!(o[k] >= 0.0)) { printf("a result that was never written\n"); exit(6); }
        sum += o[k];
      }
      if (print) printf("%u %u %a %a %a %a\n", r, s, o[0], o[1], o[2], o[3]);
    }
  if (print) printf("rounds %" PRIu64 "\n", info[0]);
  return sum;
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
  unsigned G = 0, U = 0, S = 0, R = 0;
  uint64_t nsc = 0, ncs = 0, nmembers = 0, nwords = 0;
  auto u64 = [](FILE *g, uint64_t &x) { return fscanf(g, "%" SCNu64, &x) == 1; };
  auto u32 = [](FILE *g, uint32_t &x) { return fscanf(g, "%" SCNu32, &x) == 1; };
  bool ok = fscanf(f, "%u %u %u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &G, &U, &S, &R, &nsc, &ncs, &nmembers, &nwords) == 8;
  const uint64_t cap = 1u << 22;
  ok = ok && G < cap && U < cap && (uint64_t)G * U < cap && S < cap && R < cap && nsc < cap && ncs < cap && nmembers < cap && nwords < cap;
  c.U = U;
  ok = ok && read_n(f, c.nscaf, G, u32) && read_n(f, c.sc_off, (size_t)G * U + 1, u64) && read_n(f, c.sc, nsc, u32) && read_n(f, c.ms_off, (size_t)S + 1, u64) &&
       read_n(f, c.cs_off, ncs + 1, u64) && read_n(f, c.cs_marker, nmembers, u32) && read_n(f, c.test, R, u32) && read_n(f, c.cont, R, u32) &&
       read_n(f, c.bit_off, (size_t)R + 1, u64) && read_n(f, c.bits, nwords, u32);
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_simscaf_args a = c.args();
  const int rc = ckm_simscaf_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto hit_offsets = [&](std::vector<uint64_t> &t) { t[rnd() % t.size()] = rnd() % 4 == 0 ? rnd() : rnd() % (t.back() + 3); };
  auto hit_indices = [&](std::vector<uint32_t> &t, uint64_t bound) {
    if (!t.empty()) t[rnd() % t.size()] = (uint32_t)(rnd() % 3 ? rnd() % (bound + 1) : rnd());
  };
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 10) {
        case 0: hit_offsets(d.sc_off); break;
        case 1: hit_offsets(d.ms_off); break;
        case 2: hit_offsets(d.cs_off); break;
        case 3: hit_offsets(d.bit_off); break;
        case 4: hit_indices(d.cs_marker, d.U); break;
        case 5: hit_indices(d.sc, 70); break;
        case 6: hit_indices(d.test, d.nscaf.size()); break;
        case 7: hit_indices(d.cont, d.nscaf.size()); break;
        case 8: hit_indices(d.nscaf, 70); break;
        default: if (!d.bits.empty()) d.bits[rnd() % d.bits.size()] = rnd() % 2 ? (uint32_t)rnd() : 1u << (rnd() % 32); break;
      }
    a = d.args();
    const int drc = ckm_simscaf_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
