// covwin_host_check.cpp -- TEST INFRASTRUCTURE: the library's BAM reader (bam_host.cpp) and the host executor of the CoverageWindows pass
// (tests/emu/covwin_emu.cpp: record logic, scatter into direct / diff, scan) under AddressSanitizer / UBSan
// (tests/test_covwin_sanitize.py).  The valid file is read with several batch and window sizes, then damaged copies are: a flipped
// byte, a cut, a spoiled length field.  A damaged file must be accepted or refused -- never crash, never read or write outside a buffer.
//   usage: covwin_host_check <valid.bam> <work dir> <rounds> <seed>     prints one JSON line
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

extern "C" int emu_covwin(const char *path, double min_align_per, double max_edit_dist_per, int all_reads, int64_t window, uint64_t budget, int threads,
                          int64_t *out, uint64_t cap_refs, int64_t *first, int64_t *sums, uint64_t cap_slots, uint64_t *info, char *why, uint32_t cap);

struct Result {
  std::vector<int64_t> counters, first, sums;
  uint64_t info[5];
};

static int run(const std::string &path, int64_t window, uint64_t budget, Result &r) {
  char why[512];
  r.counters.assign(4096 * 9, 0); r.first.assign(4097, 0); r.sums.assign(1 << 20, 0);
  return emu_covwin(path.c_str(), 0.98, 0.02, 0, window, budget, 3, r.counters.data(), 4096, r.first.data(), r.sums.data(), r.sums.size(), r.info, why, sizeof why);
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const std::string valid = argv[1], work = argv[2];
  const int rounds = atoi(argv[3]);
  std::mt19937_64 rng((uint64_t)atoll(argv[4]));
  Result one, again;
  uint64_t slots = 0;
  for (int64_t w : {(int64_t)1, (int64_t)7, (int64_t)100, (int64_t)5000, (int64_t)0x7fffffff}) {
    if (run(valid, w, 0, one) != 0) { fprintf(stderr, "the valid file was refused with windows of %lld\n", (long long)w); return 1; }
    slots += one.info[4];
    for (uint64_t budget : {(uint64_t)1, (uint64_t)777, (uint64_t)1 << 16}) {
      if (run(valid, w, budget, again) != 0 || again.counters != one.counters || again.first != one.first || again.sums != one.sums) {
        fprintf(stderr, "batches of %llu bytes change the result\n", (unsigned long long)budget);
        return 1;
      }
    }
  }
  if (run(valid, 0, 0, again) == 0 || run(valid, (int64_t)1 << 31, 0, again) == 0) { fprintf(stderr, "a window size out of range was accepted\n"); return 1; }
  if (run(valid, 100, 0, one) != 0) return 1;
  std::vector<uint8_t> bytes;
  {
    FILE *f = fopen(valid.c_str(), "rb");
    if (!f) return 1;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    fclose(f);
  }
  int accepted = 0, rejected = 0;
  const std::string path = work + "/damaged.bam";
  for (int r = 0; r < rounds; ++r) {
    std::vector<uint8_t> d = bytes;
    const int kind = r % 3;
    if (kind == 0) { for (int k = 0; k < 1 + r % 4; ++k) d[rng() % d.size()] ^= (uint8_t)(1 + rng() % 255); }
    else if (kind == 1) d.resize(rng() % d.size());
    else { const size_t at = rng() % (d.size() - 4); const uint32_t v = (uint32_t)rng(); memcpy(d.data() + at, &v, 4); }
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return 1;
    fwrite(d.data(), 1, d.size(), f);
    fclose(f);
    if (run(path, r % 5 ? 100 : 1, r % 2 ? 0 : 4096, again) == 0) ++accepted; else ++rejected;
  }
  printf("{\"records\": %llu, \"slots\": %llu, \"accepted\": %d, \"rejected\": %d}\n", (unsigned long long)one.info[0], (unsigned long long)slots, accepted, rejected);
  return 0;
}
