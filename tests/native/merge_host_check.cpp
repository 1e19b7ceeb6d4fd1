// merge_host_check.cpp -- TEST INFRASTRUCTURE: the host side of `checkm merge` (checkm_amd/csrc/merge_host.h: argument checks, the split
// of the rows into output batches, the lines of merger.tsv) and the host executor of its kernels (tests/emu/merge_emu.cpp) under
// AddressSanitizer + UBSan: random worlds, output batches of a single pair, count passes of one tile, refused arguments.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

extern "C" int64_t emu_merge(uint32_t nbins, uint32_t ngenes, const uint64_t *bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr, uint64_t cap_pairs,
                             uint32_t pass_rows, uint32_t *oi, uint32_t *oj, double *cols, uint64_t max_out, uint64_t *nbatches);
extern "C" uint64_t emu_merge_lines(const char *const *ids, const uint32_t *pi, const uint32_t *pj, const double *cols, uint64_t stride, uint64_t n, char *buf, uint64_t cap);
extern "C" int emu_merge_check(uint32_t nbins, uint32_t ngenes, const uint64_t *bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr, char *why, uint32_t cap);

int main() {
  std::mt19937_64 rng(20261016);
  const uint32_t shapes[][2] = {{1, 40}, {2, 64}, {63, 104}, {64, 65}, {65, 1050}, {130, 2500}, {257, 104}};
  uint64_t total = 0, batches = 0;
  for (const auto &sh : shapes) {
    const uint32_t nb = sh[0], ng = sh[1], nw = (ng + 63) / 64;
    std::vector<uint64_t> bits((size_t)nb * nw);
    std::vector<int64_t> sum(nb);
    std::vector<int32_t> nm(nb);
    for (uint32_t b = 0; b < nb; ++b) {
      int64_t members = 0;
      for (uint32_t g = 0; g < ng; ++g)
        if (rng() % 100 < 20 + b % 70) { bits[(size_t)b * nw + g / 64] |= (uint64_t)1 << (g % 64); ++members; }
      sum[b] = members + (int64_t)(rng() % 5);
      nm[b] = (int32_t)ng + (b % 3 == 0 ? 5 : 0);
    }
    const double loose[4] = {-1000, 1000, -1000, 1000}, dflt[4] = {5, 10, 50, 20};
    const uint64_t max_out = (uint64_t)nb * (nb - 1) / 2 + 1;
    std::vector<uint32_t> oi(max_out), oj(max_out);
    std::vector<double> cols(9 * max_out);
    for (int variant = 0; variant < 4; ++variant) {
      uint64_t nbat = 0;
      const int64_t k = emu_merge(nb, ng, bits.data(), sum.data(), nm.data(), variant & 1 ? dflt : loose, variant & 2 ? 1 : 0, variant & 2 ? 64 : 0, oi.data(), oj.data(),
                                  cols.data(), max_out, &nbat);
      if (k < 0 || ((variant & 1) == 0 && (uint64_t)k != max_out - 1)) { fprintf(stderr, "shape %u x %u variant %d: %lld\n", nb, ng, variant, (long long)k); return 1; }
      total += (uint64_t)k; batches += nbat;
      std::vector<std::string> names(nb);
      std::vector<const char *> ids(nb);
      for (uint32_t b = 0; b < nb; ++b) { names[b] = "bin_" + std::to_string(b); ids[b] = names[b].c_str(); }
      std::vector<char> buf((size_t)k * 160 + 16);
      const uint64_t n = emu_merge_lines(ids.data(), oi.data(), oj.data(), cols.data(), max_out, (uint64_t)k, buf.data(), buf.size());
      if (n > buf.size()) { fprintf(stderr, "lines longer than expected\n"); return 1; }
    }
    // refused arguments: nothing is read beyond what was declared
    char why[128];
    const double thr[4] = {0, 0, 0, 0};
    std::vector<int32_t> bad_n(nm); bad_n[nb - 1] = 0;
    if (emu_merge_check(nb, ng, bits.data(), sum.data(), bad_n.data(), thr, why, sizeof why) == 0) return 2;
    if (ng % 64) {
      std::vector<uint64_t> stray(bits); stray[(size_t)nb * nw - 1] |= (uint64_t)1 << 63;
      if (emu_merge_check(nb, ng, stray.data(), sum.data(), nm.data(), thr, why, sizeof why) == 0) return 3;
    }
    if (emu_merge_check(nb, 0, bits.data(), sum.data(), nm.data(), thr, why, sizeof why) == 0) return 4;
    if (emu_merge_check(nb, ng, nullptr, sum.data(), nm.data(), thr, why, sizeof why) == 0) return 5;
  }
  printf("{\"pairs\": %llu, \"batches\": %llu}\nok\n", (unsigned long long)total, (unsigned long long)batches);
  return 0;
}
