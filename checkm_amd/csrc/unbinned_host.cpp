// unbinned_host.cpp -- host side of `checkm unbinned` (additions to ABI 12): which contigs of the assembly Unbinned.run keeps
// (checkm/unbinned.py:39-68) and the two files it writes (checkm/unbinned.py:59-80), straight from the reader's buffers.  Host code only.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_set>
#include "ckm_internal.h"
#include "nucstats_host.h"
#include "unbinned_dev.h"

using namespace ckm;

extern "C" int ckm_unbinned_select(const ckm_fasta_ids *bins, const ckm_nucseq *a, int64_t min_len, uint8_t *keep, ckm_unbinned_totals *t) {
  try {
    if (!t || (a && !keep && !a->ids.empty())) throw Error(CKM_EINVAL, "NULL argument");
    *t = ckm_unbinned_totals{};
    std::unordered_set<std::string_view> binned;               // the ids stay in `bins`: the set holds views, compared byte by byte
    if (bins) {
      binned.reserve(bins->ids.size());
      for (size_t s = 0; s < bins->ids.size(); ++s) { binned.insert(std::string_view(bins->ids[s])); t->binned_bases += bins->seq_cp[s]; }
    }
    t->binned_ids = binned.size();
    if (!a) return CKM_OK;                                     // the bins' totals alone, for the log line in front of the assembly's read
    t->all_seqs = a->ids.size();
    for (size_t s = 0; s < a->ids.size(); ++s) {
      t->all_bases += a->seq_cp[s];
      const bool k = !binned.count(std::string_view(a->ids[s])) && (min_len <= 0 || a->seq_cp[s] >= (uint64_t)min_len);
      keep[s] = k ? 1 : 0;
      if (k) { t->unbinned_seqs += 1; t->unbinned_bases += a->seq_cp[s]; }
    }
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

namespace {
struct File {
  FILE *f = nullptr;
  ~File() { if (f) fclose(f); }
  void open(const char *path) {
    f = fopen(path, "wb");
    if (!f) throw Error(CKM_EIO, std::string("cannot write ") + path + ": " + strerror(errno));
    setvbuf(f, nullptr, _IOFBF, 1 << 20);
  }
  void put(const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) throw Error(CKM_EIO, std::string("write failed: ") + strerror(errno)); }
  void close() {
    FILE *g = f; f = nullptr;
    if (g && fclose(g)) throw Error(CKM_EIO, std::string("write failed: ") + strerror(errno));
  }
};
}  // namespace

extern "C" int ckm_unbinned_write(const ckm_nucseq *a, const uint8_t *keep, const uint64_t *counts, const char *seq_path, const char *stats_path, int64_t *zero_seq) {
  try {
    if (!a || !seq_path || !stats_path || !zero_seq || (!a->ids.empty() && (!keep || !counts))) throw Error(CKM_EINVAL, "NULL argument");
    *zero_seq = -1;
    for (size_t s = 0; s < a->ids.size(); ++s)
      if (keep[s] && counts[s * ub::NCOUNT + 4] != a->seq_cp[s])
        throw Error(CKM_EINVAL, "counted " + std::to_string(counts[s * ub::NCOUNT + 4]) + " code points in sequence " + a->ids[s] + ", the reader " + std::to_string(a->seq_cp[s]));
    File seq, stats;
    seq.open(seq_path); stats.open(stats_path);
    static const char header[] = "Sequence Id\tLength\tGC\n";
    stats.put(header, sizeof header - 1);
    char row[96];
    for (size_t s = 0; s < a->ids.size(); ++s) {
      if (!keep[s]) continue;
      const std::string &id = a->ids[s];
      seq.put(">", 1); seq.put(id.data(), id.size()); seq.put("\n", 1);
      seq.put(a->text.data() + a->seq_off[s], (size_t)a->seq_bytes[s]); seq.put("\n", 1);
      const uint64_t *c = counts + s * ub::NCOUNT;
      const uint64_t acgt = c[0] + c[1] + c[2] + c[3];
      if (!acgt) { *zero_seq = (int64_t)s; break; }            // the reference's ZeroDivisionError: this record is written, its row is not
      // float(g + c) * 100 / (a + c + g + t): the same three double operations, and glibc's %.2f rounds the exact binary value as Python's does
      const double gc = (double)(c[2] + c[1]) * 100 / (double)acgt;
      const int n = snprintf(row, sizeof row, "\t%llu\t%.2f\n", (unsigned long long)a->seq_cp[s], gc);
      stats.put(id.data(), id.size()); stats.put(row, (size_t)n);
    }
    seq.close(); stats.close();
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}
