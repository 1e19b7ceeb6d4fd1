// aai_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the all-pairs amino-acid identity (ckm_aai_check in aai_host.cpp, the
// packing, the batches and the pair decode of aai_dev.h) built with -fsanitize=address,undefined on the CPU.  The device pass is the
// host walk of aai_dev.h's own per-chunk step, over a buffer of exactly each batch's text.
//   <groups file> <budget bytes> <damaged tables>
// The file holds a line "G <n>" per group followed by its n rows, each behind a ':'.  Prints "check rc=<code>", one line
// "<group> <i> <j> <mismatches> <compared> <aai as %.17g>" per pair and "batches <count>"; then, <damaged tables> times, the offset
// tables with entries overwritten are checked ("damaged rc=<code>") and, where the check passes, packed and walked as well.  A caller
// owns the sizes of its arrays: the last entry of a table says how long the next array is, so a damaged last entry is only lowered.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "aai_dev.h"

namespace ckm { static std::string g_last; void set_last_error(const std::string &m) { g_last = m; } }
using namespace ckm;

static uint64_t walk(uint32_t ngroups, const std::vector<uint64_t> &gro, const std::vector<uint64_t> &ro, const std::string &text, uint64_t budget, bool print) {
  aai::Packed P;
  aai::pack(ngroups, gro.data(), ro.data(), text.data(), P);
  aai::Batch B;
  uint64_t cursor = 0, batches = 0, sum = 0;
  while (aai::next_batch(P, budget, cursor, B)) {
    std::vector<uint8_t> dev(P.text.begin() + B.text_lo, P.text.begin() + B.text_lo + B.text_bytes);
    for (uint64_t p = B.p0; p < B.p0 + B.npairs; ++p) {
      const uint32_t g = aai::find_group(P.pair_off.data(), B.g_lo, B.g_hi, p);
      const aai::Group G = P.groups[g];
      uint32_t i, j;
      aai::decode_pair(p - P.pair_off[g], G.n, i, j);
      if (!(i < j && j < G.n)) { printf("decode failed\n"); exit(5); }
      const int L = (int)G.len;
      const uint64_t stride = aai::pad16(G.len);
      const uint8_t *ri = dev.data() + (G.text_off - B.text_lo) + i * stride, *rj = dev.data() + (G.text_off - B.text_lo) + j * stride;
      std::vector<aai::Chunk> m;
      int first = aai::NO_COLUMN, last = -1;
      for (int off = 0; off < L; off += aai::LANE_BYTES) {
        uint32_t x[4], y[4];
        memcpy(x, ri + off, aai::LANE_BYTES); memcpy(y, rj + off, aai::LANE_BYTES);
        m.push_back(aai::chunk_masks(x, y, L - off));
        aai::chunk_span(m.back(), off, first, last);
      }
      int start, end, mis = 0, cmp = 0;
      aai::pair_span(first, last, L, start, end);
      for (size_t c = 0; c < m.size(); ++c) aai::chunk_count(m[c], (int)c * aai::LANE_BYTES, start, end, mis, cmp);
      if (print) printf("%u %u %u %d %d %.17g\n", g, i, j, mis, cmp, aai::identity(mis, cmp));
      sum += (uint64_t)mis + (uint64_t)cmp;
    }
    ++batches;
  }
  if (print) printf("batches %" PRIu64 "\n", batches);
  return sum;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <groups file> <budget bytes> <damaged tables>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint64_t> gro(1, 0), ro(1, 0);
  std::string text, line;
  for (int ch; (ch = fgetc(f)) != EOF;) {
    if (ch != '\n') { line.push_back((char)ch); continue; }
    if (line.size() > 1 && line[0] == 'G') gro.push_back(gro.back());
    else if (!line.empty() && line[0] == ':' && gro.size() > 1) { text.append(line, 1, std::string::npos); ro.push_back(text.size()); gro.back() += 1; }
    line.clear();
  }
  fclose(f);
  const uint32_t ngroups = (uint32_t)gro.size() - 1;
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  const int rc = ckm_aai_check(ngroups, gro.data(), ro.data(), text.data());
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", g_last.c_str());
  else walk(ngroups, gro, ro, text, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    std::vector<uint64_t> g2 = gro, r2 = ro;
    for (int hits = 1 + k % 3; hits > 0; --hits) {
      std::vector<uint64_t> &t = rnd() % 2 ? g2 : r2;
      const size_t at = rnd() % t.size();
      const uint64_t v = rnd() % 4 == 0 ? rnd() : rnd() % (t.back() + 2);
      t[at] = at + 1 == t.size() && v > t[at] ? t[at] : v;
    }
    const int drc = ckm_aai_check(ngroups, g2.data(), r2.data(), text.data());
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(ngroups, g2, r2, text, budget, false);
  }
  return 0;
}
