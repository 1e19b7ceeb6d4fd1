// cascade_plan.h -- what a search decides on the host before its first launch and after its drain: which pairs a lane owns, where the
// length-sorted order of every bin is cut into parts, which SSV blocks exist and in which order, which groups there are and how many
// entries each per-group queue gets, how large the shared tables and the two zones of the float workspace are, and what the divisors and
// floors learn from a search that overflowed.  Pure host code without HIP, without getenv and without I/O: ckm_search.hip fills a
// PlanOptions and a PlanModel per model once per call and reads the results; tests/native/cascade_plan_check.cpp compiles it alone
// (tests/test_cascade_plan_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>
#include "dev_types.h"
#include "wave_const.h"

namespace ckm {

constexpr int kSsvNone = 65;          // "SSV class" of a model beyond the 2048 nodes the SSV kernel's LDS image holds: every pair goes to the exact MSV kernel

// The tuning variables of a search, read by ckm_search.hip once per call (never cached: tests and bench.py change them between calls).
struct PlanOptions {
  uint64_t pair_budget = (uint64_t)1 << 29;     // pairs per SSV chunk (2 B of maxV each); CKM_PAIR_BUDGET overrides (tests)
  uint64_t split_min = 2000000;                 // CKM_SPLIT_MIN_PAIRS: searches below this many pairs keep one part
  const char *long_share = nullptr;             // CKM_LONG_SHARE, unparsed; null: the default shares
  uint64_t shrink = 1;                          // CKM_CAP_SHRINK (>= 1)
};

// What a model contributes to the plan (indexed by model id; ckm_search.hip fills it from the host profiles and the device models)
struct PlanModel { int cls = 0; uint32_t per_block = 1; int M = 0, fbQ = 0; int vit_cls = 0, vitx_cls = 0, fb_cls = 0; };     // cls: SSV class, per_block: sequences per SSV block

struct SeqRange { std::vector<uint32_t> lo, hi; std::vector<uint64_t> res; uint64_t tag = 0; };   // per bin: [lo, hi) of s->order, residues in it

typedef std::vector<std::vector<uint32_t>> ModelBins;                               // per model: the bins it is scanned against
typedef std::vector<std::pair<int, std::pair<size_t, size_t>>> PlanGroups;          // (key, (first block, blocks)), ascending by key, tiling the block table

// ---- the lane's models ----------------------------------------------------------------------------------------------------------
struct MW { uint32_t model; uint64_t pair_base; uint64_t npairs; };
struct LaneModels { std::vector<MW> mws; uint64_t total_pairs = 0; size_t next = 0; };      // next: index into my_models behind the last model looked at

// The models of my_models[i0 ..) that have pairs, with the base of their pairs; stops in front of the model that would take the pairs
// beyond `budget` (a single model larger than the budget is still taken).  The device-driven cascade takes them all (no budget).
inline LaneModels lane_models(const SeqRange &rng, const std::vector<uint32_t> &my_models, const ModelBins &model_bins, size_t i0 = 0, uint64_t budget = ~(uint64_t)0) {
  LaneModels lm;
  size_t i1 = i0;
  for (; i1 < my_models.size(); ++i1) {
    const uint32_t m1 = my_models[i1];
    uint64_t n = 0;
    for (uint32_t b : model_bins[m1]) n += rng.hi[b] - rng.lo[b];
    if (n == 0) continue;
    if (lm.total_pairs + n > budget && !lm.mws.empty()) break;
    lm.mws.push_back({m1, lm.total_pairs, n}); lm.total_pairs += n;
  }
  lm.next = i1;
  return lm;
}

// ---- parts by sequence length ---------------------------------------------------------------------------------------------------
// Parts by sequence length: the long sequences of every bin (a prefix of its length-sorted order) are scanned first, so that their
// chains -- every stage lasts as long as its longest sequence -- run underneath the SSV launches of the parts behind them, and what
// is left after the last SSV launch is the chain of the shortest sequences only.
// cut[k][b] .. cut[k+1][b] = part k of bin b's length-sorted order (lengths descend along it); CKM_LONG_SHARE="0.25,0.5" gives the
// shares of the residues of all parts but the last.  Two parts by default (the longest sequences holding a quarter of the residues,
// then the rest); a third part of the shortest sequences, scanned last so that only short chains are left at the end, was measured
// and does not pay: 18 more launches and chains cost what the shorter tail gains (cfg2: 86.4-88.0 ms against 85.3).
struct Parts {
  std::vector<std::vector<uint32_t>> cut;
  int nparts = 1, Lcut = 0;
  std::vector<int> Lcuts;
};

inline std::vector<double> parse_shares(const char *e) {
  std::vector<double> shares{0.25};
  if (e) {
    shares.clear();
    for (const char *q = e; *q;) {
      char *end = nullptr;
      const double v = strtod(q, &end);
      if (end == q) break;
      if (v > 0.0 && v < 1.0) shares.push_back(v);
      if (*end != ',') break;
      q = end + 1;
    }
  }
  return shares;
}

// all of every bin as the one part (the host-driven cascade, and searches below split_min)
inline Parts whole_bins(const SeqRange &rng) { Parts pt; pt.cut.push_back(rng.lo); pt.cut.push_back(rng.hi); return pt; }

inline Parts plan_parts(const SeqRange &rng, const uint32_t *order, const int32_t *len, int maxL, uint32_t nbins, uint64_t total_pairs, const PlanOptions &opt) {
  Parts pt;
  pt.cut.assign(1, rng.lo);
  const std::vector<double> shares = parse_shares(opt.long_share);
  if (total_pairs >= opt.split_min && !shares.empty()) {
    std::vector<uint64_t> by_len((size_t)maxL + 2, 0);
    uint64_t total = 0;
    for (uint32_t b = 0; b < nbins; ++b) for (uint32_t k = rng.lo[b]; k < rng.hi[b]; ++k) { const int L = len[order[k]]; by_len[L] += (uint64_t)L; total += (uint64_t)L; }
    uint64_t acc = 0; double want = 0.0; size_t si = 0;
    want = shares[0];
    for (int L = maxL; L >= 1 && si < shares.size(); --L) {
      acc += by_len[L];
      if ((double)acc >= want * (double)total) {
        if (L - 1 > 0 && (pt.Lcuts.empty() || L - 1 < pt.Lcuts.back())) pt.Lcuts.push_back(L - 1);      // part boundary: lengths > L-1 | <= L-1
        if (++si < shares.size()) want += shares[si];
      }
    }
    for (int lc : pt.Lcuts) {
      std::vector<uint32_t> c(nbins);
      for (uint32_t b = 0; b < nbins; ++b) {
        uint32_t lo = rng.lo[b], hi = rng.hi[b];                 // first position with len <= lc
        while (lo < hi) { const uint32_t m = (lo + hi) / 2; if (len[order[m]] > lc) lo = m + 1; else hi = m; }
        c[b] = lo;
      }
      pt.cut.push_back(std::move(c));
    }
    pt.nparts = (int)pt.Lcuts.size() + 1;
    if (!pt.Lcuts.empty()) pt.Lcut = pt.Lcuts[0];
  }
  pt.cut.push_back(rng.hi);
  return pt;
}

// ---- the plan key ---------------------------------------------------------------------------------------------------------------
// The block table depends only on (profiles, sequences, models and their bins): reuse the resident one when the
// previous call on this worker had the same plan (lineage_wf scans the same bins twice; bench repeats steps).
inline void key_models(std::vector<uint64_t> &key, const std::vector<MW> &mws, const ModelBins &model_bins) {
  for (auto &mw : mws) { key.push_back(0xffffffffull + mw.model); for (uint32_t b : model_bins[mw.model]) key.push_back(b); }
}
// host-driven cascade: `next` = where the chunk ends in the lane's models
inline std::vector<uint64_t> plan_key_host(uint64_t prof_uid, uint64_t seq_uid, uint64_t pair_budget, uint64_t next, uint64_t tag, const std::vector<MW> &mws, const ModelBins &model_bins) {
  std::vector<uint64_t> key{prof_uid, seq_uid, pair_budget, next, tag};
  key_models(key, mws, model_bins);
  return key;
}
// device-driven cascade: its table is cut into parts and ordered differently, so its key never equals a host-driven one
inline std::vector<uint64_t> plan_key_dev(uint64_t prof_uid, uint64_t seq_uid, uint64_t pair_budget, const Parts &pt, uint64_t tag, const std::vector<MW> &mws, const ModelBins &model_bins) {
  std::vector<uint64_t> key{prof_uid, seq_uid, pair_budget, (uint64_t)pt.Lcut, tag, 0xdeull};
  for (int lc : pt.Lcuts) key.push_back(0xc0000000ull + (uint64_t)lc);
  key_models(key, mws, model_bins);
  return key;
}

// ---- the SSV block tables and their groups --------------------------------------------------------------------------------------
// key = part * 1000 + code of the SSV launch class, the code growing with the length of the models (groups are launched heaviest first):
// 8-lane classes 100 + Q8 (models of <= 512 nodes) -> Q8, 16-lane classes Q -> 40 + Q, kSsvNone -> 105
inline int enc(int cls) { return cls >= 100 ? cls - 100 : 40 + cls; }
inline int dec(int code) { return code < 40 ? 100 + code : code - 40; }
inline int group_key(int part, int cls) { return part * 1000 + enc(cls); }
inline int group_part(int key) { return key / 1000; }
inline int group_class(int key) { return dec(key % 1000); }

struct BlockTable {
  std::vector<SsvBlockWork> work;
  PlanGroups groups;
  uint64_t pairs = 0, residues = 0, cells = 0;      // of the lane's models: pairs, residues x models, residues x model positions
};

// runs = the sequences of one (model, bin, part), already longest first
struct Run { uint32_t model, first, count; uint64_t pair0; };

// every run of the lane, in the order (model, bin, part), to fn(part, class, run); the totals of the models go to `t`
template <class F> void for_each_run(const std::vector<MW> &mws, const PlanModel *pm, const ModelBins &model_bins, const SeqRange &rng, const Parts &pt, BlockTable &t, F fn) {
  for (auto &mw : mws) {
    const int Q = pm[mw.model].cls;
    uint64_t pb = mw.pair_base;
    for (uint32_t b : model_bins[mw.model]) {
      const uint32_t o0 = rng.lo[b], n = rng.hi[b] - o0;
      for (int part = 0; part < pt.nparts; ++part) {
        const uint32_t a0 = pt.cut[part][b] - o0, a1 = pt.cut[part + 1][b] - o0;
        if (a1 > a0) fn(part, Q, Run{mw.model, o0 + a0, a1 - a0, pb + a0});
      }
      pb += n; t.residues += rng.res[b]; t.cells += rng.res[b] * (uint64_t)pm[mw.model].M;
    }
    t.pairs += mw.npairs;
  }
}

inline SsvBlockWork run_block(const Run &r, uint32_t a, uint32_t per_block) {
  SsvBlockWork w; w.model = r.model; w.list_start = r.first + a; w.count = std::min(per_block, r.count - a); w.pair_start = (uint32_t)(r.pair0 + a);
  return w;
}

// SSV block table, grouped by SSV register class = model length class (cached when the previous call on this worker had the same
// plan: lineage_wf scans the same bins twice, bench repeats steps).  Each group is one SSV launch AND one sub-cascade: its survivors
// go down their own chain of queues as soon as that launch is done, while the SSV launches of the other groups still run.
inline BlockTable block_table_dev(const std::vector<MW> &mws, const PlanModel *pm, const ModelBins &model_bins, const SeqRange &rng, const Parts &pt,
                                  const uint32_t *order, const int32_t *len) {
  // runs = the sequences of one (model, bin, part), already longest first; a launch takes the first block of every run, then the
  // second of every run, ...: its blocks come out (nearly) longest first without sorting a million of them (a block's time is set
  // by its first = longest sequence, and the few very long ones must not start last)
  BlockTable t;
  std::map<int, std::vector<Run>> runs;
  for_each_run(mws, pm, model_bins, rng, pt, t, [&](int part, int Q, const Run &r) { runs[group_key(part, Q)].push_back(r); });
  for (auto &kv : runs) {
    std::vector<Run> &rv = kv.second;
    const uint32_t per_block = pm[rv[0].model].per_block;      // (of the group's class: every model of a class has the same)
    const size_t first = t.work.size();
    std::stable_sort(rv.begin(), rv.end(), [&](const Run &x, const Run &y) { return len[order[x.first]] > len[order[y.first]]; });
    for (uint32_t a = 0;; a += per_block) {
      bool any = false;
      for (const Run &r : rv) if (a < r.count) { any = true; t.work.push_back(run_block(r, a, per_block)); }
      if (!any) break;
    }
    t.groups.push_back({kv.first, {first, t.work.size() - first}});
  }
  return t;
}

// The host-driven cascade's table: one group per SSV class (key = the class itself), blocks per (model, bin).
inline BlockTable block_table_host(const std::vector<MW> &mws, const PlanModel *pm, const ModelBins &model_bins, const SeqRange &rng,
                                   const uint32_t *order, const int32_t *len) {
  BlockTable t;
  std::map<int, std::vector<SsvBlockWork>> byQ;
  for_each_run(mws, pm, model_bins, rng, whole_bins(rng), t, [&](int, int Q, const Run &r) {
    const uint32_t per_block = pm[r.model].per_block;
    for (uint32_t a = 0; a < r.count; a += per_block) byQ[Q].push_back(run_block(r, a, per_block));
  });
  for (auto &kv : byQ) {
    // longest blocks first inside a launch (a block's time is set by its first = longest sequence): without this
    // the few very long sequences of each bin start late and leave most CUs idle at the end of every launch
    std::stable_sort(kv.second.begin(), kv.second.end(), [&](const SsvBlockWork &x, const SsvBlockWork &y) {
      return len[order[x.list_start]] > len[order[y.list_start]]; });
    t.groups.push_back({kv.first, {t.work.size(), kv.second.size()}}); t.work.insert(t.work.end(), kv.second.begin(), kv.second.end());
  }
  return t;
}

// ---- the groups' demands --------------------------------------------------------------------------------------------------------
// per group: its pairs and the Viterbi / Forward register classes of its models
struct Sub { int Q; int maxM = 0; size_t first, nblocks; uint64_t pairs = 0; bool vit[NVC] = {false}, fb[NFC] = {false};
             uint32_t cap_cand = 0, cap_nores = 0, cap_f = 0, cap_e = 0, cap_r = 0; size_t o_cand = 0, o_nores = 0, o_vq = 0, o_f = 0, o_e = 0, o_r = 0; };

inline std::vector<Sub> plan_subs(const PlanGroups &groups, const std::vector<MW> &mws, const PlanModel *pm, const ModelBins &model_bins, const Parts &pt) {
  std::vector<Sub> subs;
  std::map<int, size_t> at;
  for (auto &g : groups) { Sub sb; sb.Q = group_class(g.first); sb.first = g.second.first; sb.nblocks = g.second.second; at[g.first] = subs.size(); subs.push_back(sb); }
  for (auto &mw : mws) {
    const PlanModel &m = pm[mw.model];
    for (int part = 0; part < pt.nparts; ++part) {
      uint64_t np = 0;                                      // the model's pairs in this part
      for (uint32_t b : model_bins[mw.model]) np += pt.cut[part + 1][b] - pt.cut[part][b];
      auto it = at.find(group_key(part, m.cls));
      if (it == at.end()) continue;                         // (no sequence of this part in the model's bins)
      Sub &sb = subs[it->second]; sb.pairs += np; sb.vit[m.vit_cls] = true; sb.vit[m.vitx_cls] = true; sb.fb[m.fb_cls] = true; sb.maxM = std::max(sb.maxM, m.M);
    }
  }
  return subs;
}

// tables, queues and result buffers of a lane; capacities only grow
struct CascadeCaps { uint32_t fwork = 0, ework = 0, rwork = 0, pass = 0, reg = 0, events_f = 0, events_e = 0, seen_rwork = 0; uint64_t hens = 0;
                     uint32_t div_cand = 12, div_nores = 48, div_fwork = 160, div_ework = 256, div_rwork = 32768;        // per-group tables hold max(pairs / div, floor) entries
                     uint32_t fl_cand = 4096, fl_nores = 2048, fl_fwork = 2048, fl_ework = 1024, fl_rwork = 256; float ws_per_cell = 11.f, z1_per_pair = 64.f; };      // (z1_per_pair: bytes of workspace zone 1 per pair; like ws_per_cell it only grows, to 1.15 x what a search that overflowed asked for)

// (tests: CKM_CAP_SHRINK=n makes every table n times smaller than its share and drops the floors, to force the overflow -> host-driven path)
inline uint32_t capof(uint64_t pairs, uint32_t div, uint64_t floor_, uint64_t shrink) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(shrink > 1 ? 8 : floor_, pairs / ((uint64_t)div * shrink)), 0x7ffffff0ull);
}

struct TableSizes { size_t tot_cand = 0, tot_nores = 0, tot_f = 0, tot_e = 0, tot_r = 0; double cell_sum = 0.0; size_t ws_want = 0; };

// capacities: shares of the pairs (the divisors halve when a table overflowed on an earlier call), tables.  Fills the groups' cap_* and
// o_*, grows the lane's shared capacities and says how many bytes of float workspace the search wants within `ws_budget`.
inline TableSizes size_tables(std::vector<Sub> &subs, CascadeCaps &cp, const std::vector<MW> &mws, const PlanModel *pm, const ModelBins &model_bins,
                              uint64_t total_pairs, uint64_t shrink, uint64_t ws_budget) {
  TableSizes ts;
  for (Sub &sb : subs) {
    sb.cap_cand = capof(sb.pairs, cp.div_cand, cp.fl_cand, shrink);
    sb.cap_nores = sb.Q == kSsvNone ? (uint32_t)std::min<uint64_t>(sb.pairs + 64, 0x7ffffff0ull)     // no SSV for these models: every pair is recomputed exactly
                                    : capof(sb.pairs, cp.div_nores, cp.fl_nores, shrink);
    sb.cap_f = capof(sb.pairs, cp.div_fwork, cp.fl_fwork, shrink);
    sb.cap_e = capof(sb.pairs, cp.div_ework, cp.fl_ework, shrink);
    sb.cap_r = capof(sb.pairs, cp.div_rwork, cp.fl_rwork, shrink);
    sb.o_cand = ts.tot_cand; ts.tot_cand += sb.cap_cand; sb.o_nores = ts.tot_nores; ts.tot_nores += sb.cap_nores;
    sb.o_vq = sb.o_cand * NVC;
    sb.o_f = ts.tot_f * NFC; ts.tot_f += sb.cap_f; sb.o_e = ts.tot_e * NFC; ts.tot_e += sb.cap_e; sb.o_r = ts.tot_r * NFC; ts.tot_r += sb.cap_r;
  }
  auto grow = [](uint32_t &v, uint64_t want) { if (v < want) v = (uint32_t)std::min<uint64_t>(want, 0xfffffff0ull); };
  grow(cp.fwork, ts.tot_f); grow(cp.ework, ts.tot_e); grow(cp.rwork, ts.tot_r);
  grow(cp.pass, std::max<uint64_t>(1 << 13, ts.tot_e)); grow(cp.reg, (uint64_t)cp.ework + cp.rwork);
  grow(cp.events_f, std::max<uint64_t>(1 << 18, (uint64_t)cp.fwork * 16));
  grow(cp.events_e, std::max<uint64_t>(1 << 16, (uint64_t)cp.ework * 16));
  // (the export buffer of the ensembles is sized for the regions SEEN so far, with room -- not for the region tables' capacity, which is
  //  a floor per group times the groups; an overflow doubles it: CS_RWORK)
  cp.hens = std::max<uint64_t>(cp.hens, std::min<uint64_t>(cp.rwork, (uint64_t)4 * cp.seen_rwork + 8192) * (256 + ENS_NSAMPLES * 16 * 4 + 1024));
  // the float workspace, estimated from the cells the search is expected to fill: a marker model finds about one domain in a bin it is
  // scanned against, and a domain costs its envelope's matrix (about M rows of Mp floats, three arrays in place) -- so the demand follows
  // sum over models of (bins scanned against the model) x (Mp + 64) x Mp, whatever the number of ORFs in those bins and whichever kind
  // of search it is (43 phylogenetic markers against hundreds of bins, or a lineage's hundreds of models against a few bins).  Rounds
  // 2-4 priced it per (pair x model position), which follows the ORF count instead: one factor could not fit both kinds (round 3: 156 GB
  // allocated for 76 GB used), two factors still overshot 2x.  Measured on the 1000-bin workload (profiles/r04r_workspace_per_cell.txt):
  // 9.78-9.82 B per cell where every model is present in every bin (the 43 phylogenetic markers), 4.1-4.7 where about half of a
  // lineage's models are; the first estimate is 11 B (the first kind + 12 %).  A search that outgrows the estimate falls back once
  // (deferred regions) and leaves its measured bytes per cell (+15 %) for the next calls.
  for (auto &mw : mws) { const double Mp = (double)(pm[mw.model].fbQ * WAVE); ts.cell_sum += (double)model_bins[mw.model].size() * (Mp + 64.0) * Mp; }
  const uint64_t est = (uint64_t)(ts.cell_sum * cp.ws_per_cell + (double)total_pairs * 24.0) + ((uint64_t)256 << 20);
  ts.ws_want = (size_t)std::min<uint64_t>(std::max<uint64_t>(est, (uint64_t)1 << 30), ws_budget);
  return ts;
}

// zone 1: special rows and decoding terms of the parser items (~a few KB for ~0.3 % of the pairs: 64 B per pair until a search asked
// for more); zone 2: everything else.  In floats, of a workspace of `ws_floats`.
inline uint64_t zone1_floats(uint64_t ws_floats, uint64_t total_pairs, const CascadeCaps &cp) {
  return std::min<uint64_t>(ws_floats / 2, ((uint64_t)((double)total_pairs * cp.z1_per_pair) + ((uint64_t)64 << 20)) / 4) & ~(uint64_t)31;
}

// ---- the plan of the device-driven cascade --------------------------------------------------------------------------------------
enum PlanVerdict : int {
  PLAN_GO = 0,
  PLAN_NO_PAIRS,               // nothing to search: the lane is done
  PLAN_OVER_BUDGET,            // more pairs than one SSV pass holds: the host-driven cascade works chunk by chunk
  PLAN_TOO_MANY_GROUPS         // more than kMaxGroups: host-driven cascade
};
constexpr size_t kMaxGroups = 192;         // (grp_ev; 2 parts x (30 eight-lane + 29 sixteen-lane SSV classes + 1) at most)

// long part first; inside a part the heaviest register class first
inline std::vector<size_t> launch_order(const PlanGroups &groups, int nparts) {
  std::vector<size_t> order;
  size_t g0 = 0;                                             // groups are sorted by key = part * 1000 + class
  for (int part = 0; part < nparts; ++part) {
    size_t g1 = g0;
    while (g1 < groups.size() && group_part(groups[g1].first) == part) ++g1;
    for (size_t g = g1; g-- > g0;) order.push_back(g);
    g0 = g1;
  }
  return order;
}

struct CascadePlan {
  PlanVerdict verdict = PLAN_GO;
  std::vector<MW> mws; uint64_t total_pairs = 0;
  Parts parts;
  std::vector<uint64_t> key;
  bool resident = false;               // the key is the resident table's: `table` stays empty and `groups` are the resident ones
  BlockTable table;
  PlanGroups groups;
  std::vector<Sub> subs;
  std::vector<size_t> order;           // launch_order
};

// The plan of one lane's search.  resident_key / resident_groups: the block table the worker holds on the device, if any.
inline CascadePlan cascade_plan(uint64_t prof_uid, uint64_t seq_uid, const SeqRange &rng, const std::vector<uint32_t> &my_models, const ModelBins &model_bins,
                                const PlanModel *pm, const uint32_t *order, const int32_t *len, int maxL, uint32_t nbins, const PlanOptions &opt,
                                const std::vector<uint64_t> &resident_key, const PlanGroups &resident_groups) {
  CascadePlan pl;
  // the lane's pairs; a search with more pairs than the SSV budget goes through the host-driven cascade (it works chunk by chunk)
  { LaneModels lm = lane_models(rng, my_models, model_bins); pl.mws = std::move(lm.mws); pl.total_pairs = lm.total_pairs; }
  if (pl.total_pairs == 0) { pl.verdict = PLAN_NO_PAIRS; return pl; }
  if (pl.total_pairs > opt.pair_budget) { pl.verdict = PLAN_OVER_BUDGET; return pl; }
  pl.parts = plan_parts(rng, order, len, maxL, nbins, pl.total_pairs, opt);
  pl.key = plan_key_dev(prof_uid, seq_uid, opt.pair_budget, pl.parts, rng.tag, pl.mws, model_bins);
  pl.resident = pl.key == resident_key;
  if (pl.resident) pl.groups = resident_groups;
  else { pl.table = block_table_dev(pl.mws, pm, model_bins, rng, pl.parts, order, len); pl.groups = pl.table.groups; }
  pl.subs = plan_subs(pl.groups, pl.mws, pm, model_bins, pl.parts);
  if (pl.subs.size() > kMaxGroups) { pl.verdict = PLAN_TOO_MANY_GROUPS; return pl; }
  pl.order = launch_order(pl.groups, pl.parts.nparts);
  return pl;
}

// ---- the float stages' queue sets (queue_set.h) ---------------------------------------------------------------------------------
// The float stages run once per FLUSH and Forward class: a flush is where the trace ensembles of a sequence part are launched, behind
// the filter chains of all of the part's groups (parts beyond the third share the last flush, as they share its ensemble queue).  A
// set's members are the groups of the flush whose models reach the class, in launch order; sets come in flush order, and inside a
// flush the class with the most registers first (its launches last longest).
inline int flush_slot(int part) { return std::min(part, 3); }
struct FloatSet { int slot, cls; uint32_t first, n; };           // members[first .. first + n)
struct FloatSets { std::vector<FloatSet> sets; std::vector<uint32_t> members; };
inline FloatSets float_sets(const PlanGroups &groups, const std::vector<Sub> &subs, const std::vector<size_t> &order) {
  FloatSets fs;
  size_t a = 0;
  while (a < order.size()) {
    const int slot = flush_slot(group_part(groups[order[a]].first));
    size_t b = a;
    while (b < order.size() && flush_slot(group_part(groups[order[b]].first)) == slot) ++b;
    for (int c = NFC - 1; c >= 0; --c) {
      const uint32_t first = (uint32_t)fs.members.size();
      for (size_t k = a; k < b; ++k) if (subs[order[k]].fb[c]) fs.members.push_back((uint32_t)order[k]);
      if (fs.members.size() > first) fs.sets.push_back({slot, c, first, (uint32_t)fs.members.size() - first});
    }
    a = b;
  }
  return fs;
}

// ---- what a drained search teaches ----------------------------------------------------------------------------------------------
struct Overflow { const char *what; int group, cls; uint64_t wanted, cap; };      // a table that was too small: (group, class) -1 where there is none
struct Lesson {
  bool fits = true;
  std::vector<Overflow> over;
  uint64_t pairs_vit = 0, pairs_vit_exact = 0, n_cand = 0, n_nores = 0;
};

// h_cnt: the counter blocks ((1 + groups) x CC_SIZE: block 0 shared, block 1 + g of group g); h_tops: the four bump allocators' tops
// (zone 1, export buffer, zone 2, unused); ws_cap / ws2_cap: the floats the two zones had.  Grows `cp` for the next searches.
inline Lesson learn_from(const uint32_t *h_cnt, const unsigned long long *h_tops, const std::vector<Sub> &subs, CascadeCaps &cp, uint64_t shrink,
                         uint64_t total_pairs, double cell_sum, uint64_t ws_cap, uint64_t ws2_cap) {
  Lesson ls;
  const uint32_t n_fwork = h_cnt[CC_FWORK], n_ework = h_cnt[CC_EWORK], n_rwork = h_cnt[CC_RWORK],
                 n_pass = h_cnt[CC_PASS], n_reg = h_cnt[CC_REG], n_evf = h_cnt[CC_EVENTS], n_eve = h_cnt[CC_EVENTS_E], status = h_cnt[CC_STATUS];
  ls.fits = status == 0;
  auto over = [&](const char *what, int g, int k, uint64_t n, uint64_t cap) { ls.fits = false; ls.over.push_back({what, g, k, n, cap}); };
  auto need = [&](const char *what, uint32_t &cap, uint32_t n) { if (n > cap) { over(what, -1, -1, n, cap); cap = (uint32_t)std::min<uint64_t>((uint64_t)n + n / 4 + 1024, 0xfffffff0ull); } };
  cp.seen_rwork = std::max(cp.seen_rwork, n_rwork);
  need("fwork", cp.fwork, n_fwork); need("ework", cp.ework, n_ework); need("rwork", cp.rwork, n_rwork); need("pass", cp.pass, n_pass);
  need("reg", cp.reg, n_reg); need("events_f", cp.events_f, n_evf); need("events_e", cp.events_e, n_eve);
  // A per-group table that overflowed is sized from what the group ASKED for (round 6): its divisor follows the observed share of the
  // pairs and its floor the observed count (+25 %), so that the same kind of search fits the next time.  Rounds 2-5 halved the divisor
  // once per search -- which changes nothing where the floor is the larger term: on inputs with many multi-domain regions (paralog
  // families, low-complexity proteins: bench.py's hard_workload) the 256-entry region queues overflowed in EVERY search, and every search
  // paid the host-driven cascade (profiles/r06q_hard_workload_overflows.txt).
  // (the divisor still halves at most once per search, and only where it was the larger term: a small group's share says nothing about
  //  the large ones -- regions follow the domains present, not the pairs scanned)
  uint32_t halved = 0;
  auto learn = [&](int kind, uint32_t &div, uint32_t &floor_, uint64_t pairs, uint64_t want) {
    const uint64_t w = want + want / 4 + 16;
    if ((pairs / std::max<uint64_t>(1, (uint64_t)div * shrink) >= floor_ || shrink > 1) && !((halved >> kind) & 1u)) { div = std::max<uint32_t>(1, div / 2); halved |= 1u << kind; }
    if (shrink == 1) floor_ = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(floor_, w), 1u << 14);
    // More than the floor may become (every group pays the floor, so it stays small): then the group's SHARE has to give it the entries,
    // whatever the larger term was -- else max(pairs / div, floor) stays below `want` and this kind of search overflows in every call.  A
    // group that asks for more entries than it has pairs (several envelopes or regions per pair) gets them from the floor after all.
    if (shrink == 1 && w > (1u << 14)) {
      const uint64_t d = pairs / w;
      if (d >= 1) div = (uint32_t)std::min<uint64_t>(div, d);
      else { div = 1; floor_ = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(floor_, w), 1u << 20); }
    }
  };
  for (size_t g = 0; g < subs.size(); ++g) {
    const uint32_t *c = h_cnt + (1 + g) * CC_SIZE; const Sub &sb = subs[g];
    ls.n_cand += c[CC_CAND]; ls.n_nores += c[CC_NORES];
    if (c[CC_CAND] > sb.cap_cand) { over("cand", (int)g, -1, c[CC_CAND], sb.cap_cand); learn(0, cp.div_cand, cp.fl_cand, sb.pairs, c[CC_CAND]); }
    if (c[CC_NORES] > sb.cap_nores) { over("nores", (int)g, -1, c[CC_NORES], sb.cap_nores); if (sb.Q != kSsvNone) learn(1, cp.div_nores, cp.fl_nores, sb.pairs, c[CC_NORES]); }
    for (int k = 0; k < NVC; ++k) {
      ls.pairs_vit += c[CC_VQ + k]; ls.pairs_vit_exact += c[CC_VXQ + k];
      const uint32_t v = std::max(c[CC_VQ + k], c[CC_VXQ + k]);
      if (v > sb.cap_cand) { over("vq", (int)g, k, v, sb.cap_cand); learn(0, cp.div_cand, cp.fl_cand, sb.pairs, v); }
    }
    for (int k = 0; k < NFC; ++k) {
      const uint32_t f = std::max(c[CC_FQ + k], c[CC_BQ + k]);
      if (f > sb.cap_f) { over("fq", (int)g, k, f, sb.cap_f); learn(2, cp.div_fwork, cp.fl_fwork, sb.pairs, f); }
      if (c[CC_EQ + k] > sb.cap_e) { over("eq", (int)g, k, c[CC_EQ + k], sb.cap_e); learn(3, cp.div_ework, cp.fl_ework, sb.pairs, c[CC_EQ + k]); }
      if (c[CC_RQ + k] > sb.cap_r) { over("rq", (int)g, k, c[CC_RQ + k], sb.cap_r); learn(4, cp.div_rwork, cp.fl_rwork, sb.pairs, c[CC_RQ + k]); }
    }
  }
  if (status & CS_RWORK) cp.hens *= 2;
  // zone 2 ran out (regions were deferred to the host): size the workspace from what this search asked for, for the next calls
  // the bump allocator counts every request, granted or not: after an overflow the search's whole demand is known, and the next one of its
  // kind gets that (+15 %) instead of a blind x1.5
  // (zone 1 the same way, per pair: where most pairs are hits -- a small database of families that every protein carries -- 64 B per
  //  pair is a third of the demand, and without this such a search took the host-driven cascade in every call)
  // (never shrinks; z1 is also held to half of the workspace: where THAT is the smaller term the search asks for more than the workspace
  //  budget gives and stays host-driven -- the trace says so)
  if (h_tops[0] > ws_cap) cp.z1_per_pair = std::max(cp.z1_per_pair, (float)(1.15 * (double)h_tops[0] * 4.0 / (double)std::max<uint64_t>(total_pairs, 1)));
  if (h_tops[2] > ws2_cap)
    cp.ws_per_cell = std::max(cp.ws_per_cell, (float)(1.15 * (double)(h_tops[2] + ws_cap) * 4.0 / std::max(cell_sum, 1.0)));
  return ls;
}

}  // namespace ckm
