// unbinned_host_check.cpp -- TEST INFRASTRUCTURE: the host code of `checkm unbinned` (the id reader ckm_fasta_ids_read in
// nucstats_host.cpp, ckm_unbinned_select and ckm_unbinned_write in unbinned_host.cpp, the tile geometry of unbinned_dev.h) built with
// -fsanitize=address,undefined on the CPU and fed the files named on the command line.  The device count is the host walk of
// unbinned_dev.h's own per-word step.
//   <min_len> <out fasta> <out stats> <assembly> [<bin> ...]
// prints "ids rc=<code>" and, for rc=0, "<nseq> <nfiles>" and one line "<id>\t<bytes>\t<code points>" per sequence of the bins, then
// "assembly rc=<code>", "select <the six totals>", the keep flags, "write rc=<code> zero=<index>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "nucstats_host.h"
#include "unbinned_dev.h"

namespace ckm { static std::string g_last; void set_last_error(const std::string &m) { g_last = m; } }
using namespace ckm;

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s <min_len> <out fasta> <out stats> <assembly> [<bin> ...]\n", argv[0]); return 2; }
  const int64_t min_len = strtoll(argv[1], nullptr, 10);
  ckm_fasta_ids *ids = nullptr;
  const int irc = ckm_fasta_ids_read(argv + 5, (uint32_t)(argc - 5), &ids);
  printf("ids rc=%d\n", irc);
  if (irc) { printf("error: %s\n", g_last.c_str()); return 0; }
  ckm_fasta_ids_view v;
  if (ckm_fasta_ids_view_get(ids, &v)) return 3;
  printf("%u %u\n", v.nseq, v.nfiles);
  for (uint32_t s = 0; s < v.nseq; ++s) printf("%s\t%" PRIu64 "\t%" PRIu64 "\n", v.seq_ids[s], v.seq_bytes[s], v.seq_cp[s]);
  ckm_nucseq *a = nullptr;
  const char *paths[1] = {argv[4]};
  const int arc = ckm_nucseq_read(paths, 1, &a);
  printf("assembly rc=%d\n", arc);
  if (arc) { printf("error: %s\n", g_last.c_str()); ckm_fasta_ids_free(ids); return 0; }
  const uint32_t nseq = (uint32_t)a->seq_off.size();
  std::vector<uint8_t> keep(nseq + 1, 0);
  ckm_unbinned_totals t;
  if (ckm_unbinned_select(ids, a, min_len, keep.data(), &t)) return 4;
  printf("select %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", t.binned_ids, t.binned_bases, t.all_seqs, t.all_bases, t.unbinned_seqs, t.unbinned_bases);
  for (uint32_t s = 0; s < nseq; ++s) printf("%d", keep[s]);
  printf("\n");
  // the count: tiles of 48 bytes in batches of 64, every batch packed into a buffer of exactly its bytes
  std::vector<ub::HostTile> tiles;
  std::vector<uint64_t> first_tile;
  std::vector<uint32_t> kept;
  ub::make_tiles(a->seq_off.data(), a->seq_bytes.data(), keep.data(), nseq, 48, tiles, first_tile, kept);
  std::vector<uint32_t> rows(tiles.size() * ub::NCOUNT + 1, 0);
  std::vector<uint64_t> counts((size_t)nseq * ub::NCOUNT + 1, 0);
  ub::Batch B;
  uint64_t cursor = 0;
  while (ub::next_batch(tiles, 64, cursor, B)) {
    std::vector<uint8_t> dev(B.bytes);
    for (const ub::Span &S : B.spans) memcpy(dev.data() + S.dst, a->text.data() + S.src, S.bytes);
    for (size_t k = 0; k < B.tiles.size(); ++k)
      for (uint32_t off = 0; off < B.tiles[k].len; off += ub::LANE_BYTES) {
        uint32_t w[4];
        memcpy(w, dev.data() + B.tiles[k].start + off, ub::LANE_BYTES);
        const uint32_t rem = B.tiles[k].len - off;
        ub::lane_counts(w, rem >= 16 ? 16 : (int)rem, &rows[(B.t0 + k) * ub::NCOUNT]);
      }
  }
  for (size_t k = 0; k < kept.size(); ++k) ub::sum_rows(rows.data(), first_tile[k], first_tile[k + 1], &counts[(size_t)kept[k] * ub::NCOUNT]);
  int64_t zero = -2;
  const int wrc = ckm_unbinned_write(a, keep.data(), counts.data(), argv[2], argv[3], &zero);
  printf("write rc=%d zero=%" PRId64 "\n", wrc, zero);
  if (wrc) printf("error: %s\n", g_last.c_str());
  ckm_nucseq_free(a);
  ckm_fasta_ids_free(ids);
  return 0;
}
