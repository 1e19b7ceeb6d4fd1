// markerset_host_check.cpp -- TEST INFRASTRUCTURE: the host code of MarkerSetBuilder (ckm_mset_check in markerset_host.cpp; the packing,
// the rounds, the tile lists and the batch cuts of markerset_dev.h, walked by the host executor of tests/emu/markerset_emu.cpp, which this
// file includes) built with -fsanitize=address,undefined on the CPU.
//   <table file> <budget bytes> <damaged tables>
// The file holds whitespace-separated numbers: G C NQ D thr; G * C count classes; G * C + 1 offsets; the positions; then per query its
// genome count and genomes, its marker count and markers, its two marker-pass thresholds.  Prints "check rc=<code>", one line
// "<query> <i> <j> <count>" per reported pair, "batches <n> rounds <n> tests <n>" and one line "flags <query> <bytes as hex>" per query;
// then, <damaged tables> times, the tables with entries overwritten are checked ("damaged rc=<code>") and, where the check passes, walked
// as well.  A caller owns the sizes of its arrays: the last entry of an offset table says how long the next array is, so a damaged last
// entry is only lowered.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "../emu/markerset_emu.cpp"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  uint32_t G = 0, C = 0, nq = 0;
  double D = 0, thr = 0;
  std::vector<uint8_t> cls;
  std::vector<uint64_t> pos_off, qg_off, qm_off;
  std::vector<int64_t> pos;
  std::vector<uint32_t> qg, qm;
  std::vector<double> tU, tS;
  int check() const {
    return ckm_mset_check(G, C, cls.data(), pos_off.data(), pos.data(), nq, qg_off.data(), qg.data(), qm_off.data(), qm.data(), D);
  }
};

static uint64_t walk(const Call &c, uint64_t budget, bool print) {
  uint64_t info[4] = {0, 0, 0, 0}, sum = 0;
  const int rc = emu_mset_colocated(c.G, c.C, c.cls.data(), c.pos_off.data(), c.pos.data(), c.nq, c.qg_off.data(), c.qg.data(), c.qm_off.data(), c.qm.data(), c.D, c.thr,
                                    budget, info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  std::vector<uint64_t> pair_off((size_t)c.nq + 1);
  std::vector<uint32_t> pi(info[0] + 1), pj(info[0] + 1), pc(info[0] + 1);
  emu_mset_fetch(pair_off.data(), pi.data(), pj.data(), pc.data());
  for (uint32_t q = 0; q < c.nq; ++q)
    for (uint64_t k = pair_off[q]; k < pair_off[q + 1]; ++k) {
      const uint64_t nm = c.qm_off[q + 1] - c.qm_off[q];
      if (!(pi[k] < pj[k] && pj[k] < nm)) { printf("a pair outside its query\n"); exit(6); }
      if (print) printf("%u %u %u %u\n", q, pi[k], pj[k], pc[k]);
      sum += pc[k];
    }
  if (print) printf("batches %" PRIu64 " rounds %" PRIu64 " tests %" PRIu64 "\n", info[1], info[2], info[3]);
  std::vector<uint8_t> flag((size_t)c.nq * c.C + 1);
  std::vector<uint32_t> counts((size_t)c.nq * c.C * 3 + 1);
  if (emu_mset_markers(c.G, c.C, c.cls.data(), c.pos_off.data(), c.pos.data(), c.nq, c.qg_off.data(), c.qg.data(), c.tU.data(), c.tS.data(), flag.data(), counts.data())) {
    printf("marker walk failed\n"); exit(7);
  }
  for (uint32_t q = 0; q < c.nq; ++q) {
    if (print) printf("flags %u ", q);
    for (uint32_t f = 0; f < c.C; ++f) {
      if (print) printf("%x", flag[(size_t)q * c.C + f]);
      sum += flag[(size_t)q * c.C + f] + counts[((size_t)q * c.C + f) * 3];
    }
    if (print) printf("\n");
  }
  return sum;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <table file> <budget bytes> <damaged tables>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  bool ok = fscanf(f, "%u %u %u %lf %lf", &c.G, &c.C, &c.nq, &c.D, &c.thr) == 5 && (uint64_t)c.G * c.C < (1u << 24) && c.nq < (1u << 20);
  const size_t cells = ok ? (size_t)c.G * c.C : 0;
  c.cls.resize(cells + 1); c.pos_off.resize(cells + 1);
  for (size_t k = 0; ok && k < cells; ++k) { unsigned v = 0; ok = fscanf(f, "%u", &v) == 1; c.cls[k] = (uint8_t)v; }
  for (size_t k = 0; ok && k <= cells; ++k) ok = fscanf(f, "%" SCNu64, &c.pos_off[k]) == 1;
  ok = ok && c.pos_off[cells] < (1u << 24);
  c.pos.resize(ok ? c.pos_off[cells] + 1 : 1);
  for (size_t k = 0; ok && k + 1 < c.pos.size(); ++k) ok = fscanf(f, "%" SCNd64, &c.pos[k]) == 1;
  c.qg_off.assign(1, 0); c.qm_off.assign(1, 0);
  for (uint32_t q = 0; ok && q < c.nq; ++q) {
    unsigned n = 0, v = 0;
    double tu = 0, ts = 0;
    ok = fscanf(f, "%u", &n) == 1 && n < (1u << 20);
    for (unsigned k = 0; ok && k < n; ++k) { ok = fscanf(f, "%u", &v) == 1; c.qg.push_back(v); }
    c.qg_off.push_back(c.qg.size());
    ok = ok && fscanf(f, "%u", &n) == 1 && n < (1u << 20);
    for (unsigned k = 0; ok && k < n; ++k) { ok = fscanf(f, "%u", &v) == 1; c.qm.push_back(v); }
    c.qm_off.push_back(c.qm.size());
    ok = ok && fscanf(f, "%lf %lf", &tu, &ts) == 2;
    c.tU.push_back(tu); c.tS.push_back(ts);
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed table file\n"); return 2; }
  c.qg.push_back(0); c.qm.push_back(0); c.tU.push_back(0); c.tS.push_back(0);      // (never an empty array's data())
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  const int rc = c.check();
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto hit_offsets = [&](std::vector<uint64_t> &t) {
    const size_t at = rnd() % t.size();
    const uint64_t v = rnd() % 4 == 0 ? rnd() : rnd() % (t.back() + 2);
    t[at] = at + 1 == t.size() && v > t[at] ? t[at] : v;
  };
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 7) {
        case 0: hit_offsets(d.pos_off); break;
        case 1: hit_offsets(d.qg_off); break;
        case 2: hit_offsets(d.qm_off); break;
        case 3: d.qg[rnd() % d.qg.size()] = (uint32_t)(rnd() % 3 ? rnd() % (d.G + 2) : rnd()); break;
        case 4: d.qm[rnd() % d.qm.size()] = (uint32_t)(rnd() % 3 ? rnd() % (d.C + 2) : rnd()); break;
        case 5: d.cls[rnd() % d.cls.size()] = (uint8_t)(rnd() % 5); break;
        default: d.pos[rnd() % d.pos.size()] = rnd() % 3 ? (int64_t)(rnd() % (1ull << 32)) - 1000 : (int64_t)rnd(); break;
      }
    const int drc = d.check();
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
