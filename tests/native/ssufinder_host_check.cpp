// ssufinder_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the nucleotide model scan (ckm_nhmm_check in nhmm_host.cpp; the check,
// the tile cuts, the recurrence, the compaction and the hit rule of nhmm_dev.h, walked by its host executor through
// tests/emu/ssufinder_emu.cpp, which this file includes) built with -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated integers: nmodels stride overlap strands nseq; nmodels node counts; nmodels thresholds; the
// emissions (4 M per model); the transitions (7 M per model); nseq lengths; the bytes of every sequence.  Prints "check rc=<code>", one
// line "r <model> <seq> <strand> <row> <start> <score>" per reported row, "h <model> <seq> <strand> <from> <to> <score>" per hit and
// "batches <n>"; then, <damaged calls> times, the call with entries overwritten is checked ("damaged rc=<code>") and, where the check
// passes, walked as well ("walk rc=<code>": 0, or a refusal of the sequences).  Every array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "../emu/ssufinder_emu.cpp"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  std::vector<uint32_t> M;
  std::vector<uint64_t> tab_off, seq_off, seq_bytes;
  std::vector<int32_t> emis, trans, thr;
  std::vector<char> text;
  uint32_t stride = 0, overlap = 0, strands = 0;
  uint64_t ntab = 0;
  ckm_nhmm_args args() const {
    return ckm_nhmm_args{(uint32_t)M.size(), M.data(), tab_off.data(), emis.data(), trans.data(), ntab, thr.data(), stride, overlap, strands};
  }
};

static int walk(const Call &c, uint64_t budget, bool print) {
  const ckm_nhmm_args a = c.args();
  ckm_nhmm_result *r = nullptr;
  int64_t info[5] = {0, 0, 0, 0, 0};
  const int rc = emu_nhmm_run(&a, c.text.data(), c.seq_off.data(), c.seq_bytes.data(), (uint32_t)c.seq_off.size(), budget, &r, info);
  if (rc) return rc;
  ckm_nhmm_columns k;
  emu_nhmm_columns(r, &k);
  for (uint64_t i = 0; i < k.nrows; ++i) {
    if (k.row_seq[i] >= c.seq_off.size() || k.row_pos[i] < 1 || k.row_pos[i] > c.seq_bytes[k.row_seq[i]] || k.row_start[i] < 1 || k.row_start[i] > k.row_pos[i]) { printf("a row out of range\n"); exit(6); }
    if (print) printf("r %u %u %u %u %u %d\n", k.row_model[i], k.row_seq[i], k.row_strand[i], k.row_pos[i], k.row_start[i], k.row_score[i]);
  }
  for (uint64_t i = 0; i < k.nhits; ++i) {
    if (k.hit_from[i] < 1 || k.hit_from[i] > k.hit_to[i] || k.hit_to[i] > c.seq_bytes[k.hit_seq[i]]) { printf("a hit out of range\n"); exit(6); }
    if (print) printf("h %u %u %u %u %u %d\n", k.hit_model[i], k.hit_seq[i], k.hit_strand[i], k.hit_from[i], k.hit_to[i], k.hit_score[i]);
  }
  if (print) printf("batches %" PRId64 "\n", info[3]);
  emu_nhmm_free(r);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  unsigned nm = 0, nseq = 0;
  bool ok = fscanf(f, "%u %u %u %u %u", &nm, &c.stride, &c.overlap, &c.strands, &nseq) == 5 && nm < 64 && nseq < 4096;
  auto i64 = [&](long long &x) { return fscanf(f, "%lld", &x) == 1; };
  long long v = 0;
  c.tab_off.push_back(0);
  for (unsigned m = 0; ok && m < nm; ++m) { ok = i64(v) && v >= 0 && v < 8192; c.M.push_back((uint32_t)v); c.tab_off.push_back(c.tab_off.back() + (uint64_t)v); }
  c.ntab = c.tab_off.back();
  for (unsigned m = 0; ok && m < nm; ++m) { ok = i64(v); c.thr.push_back((int32_t)v); }
  for (uint64_t k = 0; ok && k < 4 * c.ntab; ++k) { ok = i64(v); c.emis.push_back((int32_t)v); }
  for (uint64_t k = 0; ok && k < 7 * c.ntab; ++k) { ok = i64(v); c.trans.push_back((int32_t)v); }
  for (unsigned s = 0; ok && s < nseq; ++s) { ok = i64(v) && v >= 0 && v < (1 << 20); c.seq_off.push_back(c.text.size()); c.seq_bytes.push_back((uint64_t)v); c.text.resize(c.text.size() + (size_t)v); }
  for (size_t k = 0; ok && k < c.text.size(); ++k) { ok = i64(v) && v >= 0 && v < 256; c.text[k] = (char)v; }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_nhmm_args a = c.args();
  const int rc = ckm_nhmm_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else printf("walk rc=%d\n", walk(c, budget, true));
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  const int32_t bad[] = {0, 1, -1, 2048, 2049, -(1 << 21), -(1 << 21) - 1, INT32_MAX, INT32_MIN, -(1 << 20), -(1 << 20) - 1, 5000};
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 9) {
        case 0: if (!d.M.empty()) d.M[rnd() % d.M.size()] = (uint32_t)(rnd() % 3 ? rnd() % 4096 : rnd()); break;
        case 1: d.tab_off[rnd() % d.tab_off.size()] = rnd() % 4 ? rnd() % (d.ntab + 3) : rnd(); break;
        case 2: if (!d.thr.empty()) d.thr[rnd() % d.thr.size()] = bad[rnd() % 12]; break;
        case 3: if (!d.emis.empty()) d.emis[rnd() % d.emis.size()] = bad[rnd() % 12]; break;
        case 4: if (!d.trans.empty()) d.trans[rnd() % d.trans.size()] = bad[rnd() % 12]; break;
        case 5: d.stride = (uint32_t)(rnd() % 3 ? rnd() % 100 : rnd()); break;
        case 6: d.overlap = (uint32_t)(rnd() % 3 ? rnd() % 100 : rnd()); d.strands = (uint32_t)(rnd() % 5); break;
        case 7: d.ntab = rnd() % 2 ? d.ntab + 1 : rnd(); break;
        default: if (!d.text.empty()) d.text[rnd() % d.text.size()] = (char)rnd(); break;
      }
    a = d.args();
    const int drc = ckm_nhmm_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) printf("damaged walk rc=%d\n", walk(d, budget, false));
  }
  return 0;
}
