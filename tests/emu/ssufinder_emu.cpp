// ssufinder_emu.cpp -- TEST INFRASTRUCTURE: the score system, the check, the tile cuts, the compaction order and the hit rule of the
// nucleotide model scan (checkm_amd/csrc/nhmm_dev.h) compiled by g++ against its HOST executor (nhmm::run_host: the recurrence row by
// row as the header states it), so that the CPU test suite runs the definition the kernels of kernels_nhmm.hip are compared with.  The
// row buffer of a batch starts from a poison pattern, so that a slot that was never written shows.  Nothing in checkm_amd loads this.
#include <string>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/nhmm_dev.h"

using namespace ckm;

namespace {
nhmm::Args args_of(const ckm_nhmm_args *a) {
  return nhmm::Args{a->nmodels, a->M, a->tab_off, a->emis, a->trans, a->ntab, a->min_score, a->stride, a->overlap, a->strands};
}
}  // namespace

// 0, or nhmm::ARGS_INVALID / nhmm::ARGS_RANGE
extern "C" int emu_nhmm_check(const ckm_nhmm_args *a) {
  std::string why;
  return a ? nhmm::check(args_of(a), why) : nhmm::ARGS_INVALID;
}

// info[0..3] = tiles, launches, cells, batches; info[4] = the sequence a refusal names (or -1)
extern "C" int emu_nhmm_run(const ckm_nhmm_args *a, const char *text, const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, uint64_t budget_bytes,
                            ckm_nhmm_result **out, int64_t *info) {
  std::string why;
  nhmm::Info I;
  ckm_nhmm_result *r = new ckm_nhmm_result;
  int64_t refused = -1;
  const int rc = nhmm::run_host(args_of(a), nhmm::Seqs{text, seq_off, seq_bytes, nseq}, budget_bytes, r->rows, r->hits, I, refused, why);
  info[0] = (int64_t)I.tiles; info[1] = (int64_t)I.launches; info[2] = (int64_t)I.cells; info[3] = (int64_t)I.batches; info[4] = refused;
  if (rc) { delete r; r = nullptr; }
  *out = r;
  return rc;
}

extern "C" void emu_nhmm_columns(const ckm_nhmm_result *r, ckm_nhmm_columns *out) {
  const nhmm::Rows &w = r->rows;
  const nhmm::Hits &h = r->hits;
  *out = ckm_nhmm_columns{w.size(), w.model.data(), w.seq.data(), w.strand.data(), w.pos.data(), w.start.data(), w.score.data(),
                          h.size(), h.model.data(), h.seq.data(), h.strand.data(), h.from.data(), h.to.data(), h.score.data()};
}

extern "C" void emu_nhmm_free(ckm_nhmm_result *r) { delete r; }

extern "C" int emu_nhmm_tbm(uint32_t M) { return nhmm::tbm_of(M); }

// the hit rule on the reported rows of one (model, sequence, strand) group of a sequence of L bases: returns the number of hits,
// from / to / score into the caller's arrays of n entries
extern "C" int emu_nhmm_hits(uint32_t n, uint64_t L, uint32_t strand, const uint32_t *start, const uint32_t *row, const int32_t *score, uint32_t *from, uint32_t *to, int32_t *hscore) {
  nhmm::Rows r;
  for (uint32_t k = 0; k < n; ++k) { r.model.push_back(0); r.seq.push_back(0); r.strand.push_back(strand); r.pos.push_back(row[k]); r.start.push_back(start[k]); r.score.push_back(score[k]); }
  const uint64_t off = 0;
  nhmm::Hits h;
  nhmm::hits_host(nhmm::Seqs{nullptr, &off, &L, 1}, r, h);
  for (size_t k = 0; k < h.size(); ++k) { from[k] = h.from[k]; to[k] = h.to[k]; hscore[k] = h.score[k]; }
  return (int)h.size();
}
