// coverage_host_check.cpp -- TEST INFRASTRUCTURE: the library's BAM reader (bam_host.cpp) and the host executor of the coverage pass
// (tests/emu/coverage_emu.cpp) under AddressSanitizer / UBSan (tests/test_coverage_sanitize.py).  The valid file is read with several
// batch sizes, then damaged copies are: a flipped byte, a cut, a spoiled length field.  A damaged file must be accepted or refused --
// never crash, never read outside a buffer.
//   usage: coverage_host_check <valid.bam> <work dir> <rounds> <seed>     prints one JSON line
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

extern "C" int emu_coverage(const char *path, double min_align_per, double max_edit_dist_per, double min_qc, int all_reads, uint64_t budget, int threads,
                            int64_t *out, uint64_t cap_refs, uint64_t *info, char *why, uint32_t cap);
extern "C" int emu_bam_scan(const char *path, uint64_t budget, int threads, char *names, uint32_t cap_names, int64_t *lengths, uint64_t cap_refs, uint64_t *offsets, uint64_t cap_off,
                            uint64_t *info, char *why, uint32_t cap);

static int run(const std::string &path, uint64_t budget, std::vector<int64_t> &out, uint64_t *info) {
  char why[512];
  out.assign(4096 * 9, 0);
  return emu_coverage(path.c_str(), 0.98, 0.02, 15, 0, budget, 3, out.data(), 4096, info, why, sizeof why);
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const std::string valid = argv[1], work = argv[2];
  const int rounds = atoi(argv[3]);
  std::mt19937_64 rng((uint64_t)atoll(argv[4]));
  std::vector<int64_t> first, again;
  uint64_t info[4], info2[4];
  if (run(valid, 0, first, info) != 0) { fprintf(stderr, "the valid file was refused\n"); return 1; }
  for (uint64_t budget : {(uint64_t)1, (uint64_t)777, (uint64_t)1 << 16}) {
    if (run(valid, budget, again, info2) != 0 || again != first || info2[0] != info[0]) { fprintf(stderr, "batches of %llu bytes change the result\n", (unsigned long long)budget); return 1; }
  }
  std::vector<char> names(1 << 16);
  std::vector<int64_t> lengths(4096);
  std::vector<uint64_t> offsets(1 << 20);
  char why[512];
  if (emu_bam_scan(valid.c_str(), 0, 2, names.data(), (uint32_t)names.size(), lengths.data(), lengths.size(), offsets.data(), offsets.size(), info2, why, sizeof why) != 0) return 1;
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
    if (run(path, r % 2 ? 0 : 4096, again, info2) == 0) ++accepted; else ++rejected;
  }
  printf("{\"records\": %llu, \"accepted\": %d, \"rejected\": %d}\n", (unsigned long long)info[0], accepted, rejected);
  return 0;
}
