// cascade_plan_check.cpp -- TEST INFRASTRUCTURE: the search's host-side plan (csrc/cascade_plan.h) built with -fsanitize=address,undefined
// on the CPU.  Reads one case from the text file named on the command line and prints the plan as one JSON object.
// The case is a list of records, each a keyword and its numbers:
//   opt <pair_budget> <split_min> <shrink> <long_share | ->      ws <budget bytes> <floats held>
//   len <n> <L> ...        order <n> <seq> ...        bins <n> { <lo> <hi> <residues> } ...
//   models <n> { <cls> <per_block> <M> <fbQ> <vit_cls> <vitx_cls> <fb_cls> <nbins> <bin> ... } ...        lane <n> <model> ...
//   caps <the 19 integer fields of CascadeCaps in order> <ws_per_cell> <z1_per_pair>
//   cnt <block> <counter> <value>       (block 0: shared, 1 + g: group g; any number of these)        tops <t0> <t1> <t2> <t3>
//   blocks <0|1>           (print the block tables)
// With a `cnt` or `tops` record the lesson of a drained search is printed too, and the capacities it leaves.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include "cascade_plan.h"

using namespace ckm;

template <class T> static void list(const std::vector<T> &v) {
  printf("[");
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
  printf("]");
}
template <class T> static void arr(const char *name, const std::vector<T> &v) { printf("\"%s\":", name); list(v); printf(","); }
static void key(const char *name, const std::vector<uint64_t> &v) {
  printf("\"%s\":[", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%" PRIu64, i ? "," : "", v[i]);
  printf("],");
}
static void table(const BlockTable &t, const PlanGroups &groups, bool blocks) {
  printf("\"groups\":[");
  for (size_t g = 0; g < groups.size(); ++g) printf("%s[%d,%zu,%zu]", g ? "," : "", groups[g].first, groups[g].second.first, groups[g].second.second);
  printf("],\"pairs\":%" PRIu64 ",\"residues\":%" PRIu64 ",\"cells\":%" PRIu64 ",\"nblocks\":%zu,\"blocks\":[", t.pairs, t.residues, t.cells, t.work.size());
  if (blocks) for (size_t i = 0; i < t.work.size(); ++i) printf("%s[%u,%u,%u,%u]", i ? "," : "", t.work[i].model, t.work[i].list_start, t.work[i].count, t.work[i].pair_start);
  printf("]");
}
static void mws_out(const std::vector<MW> &mws) {
  printf("\"mws\":[");
  for (size_t i = 0; i < mws.size(); ++i) printf("%s[%u,%" PRIu64 ",%" PRIu64 "]", i ? "," : "", mws[i].model, mws[i].pair_base, mws[i].npairs);
  printf("],");
}
static void caps_out(const char *name, const CascadeCaps &c, const char *end) {
  printf("\"%s\":{\"fwork\":%u,\"ework\":%u,\"rwork\":%u,\"pass\":%u,\"reg\":%u,\"events_f\":%u,\"events_e\":%u,\"seen_rwork\":%u,\"hens\":%" PRIu64 ","
         "\"div_cand\":%u,\"div_nores\":%u,\"div_fwork\":%u,\"div_ework\":%u,\"div_rwork\":%u,\"fl_cand\":%u,\"fl_nores\":%u,\"fl_fwork\":%u,\"fl_ework\":%u,\"fl_rwork\":%u,"
         "\"ws_per_cell\":%.9g,\"z1_per_pair\":%.9g}%s", name, c.fwork, c.ework, c.rwork, c.pass, c.reg, c.events_f, c.events_e, c.seen_rwork, c.hens,
         c.div_cand, c.div_nores, c.div_fwork, c.div_ework, c.div_rwork, c.fl_cand, c.fl_nores, c.fl_fwork, c.fl_ework, c.fl_rwork, (double)c.ws_per_cell, (double)c.z1_per_pair, end);
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  PlanOptions opt; std::string share; bool has_share = false;
  uint64_t ws_budget = (uint64_t)8 << 30, ws_floats = 0;
  std::vector<int32_t> len; std::vector<uint32_t> order, lane;
  SeqRange rng; std::vector<PlanModel> pm; ModelBins model_bins;
  CascadeCaps cp;
  struct Cnt { uint64_t block, k, v; }; std::vector<Cnt> cnts;
  unsigned long long tops[4] = {0, 0, 0, 0};
  bool drained = false, blocks = true;
  auto bad = [&](const char *what) { fprintf(stderr, "bad case file: %s\n", what); return 2; };
  std::string kw;
  while (in >> kw) {
    size_t n = 0;
    if (kw == "opt") {
      if (!(in >> opt.pair_budget >> opt.split_min >> opt.shrink >> share)) return bad("opt");
      has_share = share != "-";
    } else if (kw == "ws") { if (!(in >> ws_budget >> ws_floats)) return bad("ws"); }
    else if (kw == "len") { if (!(in >> n)) return bad("len"); len.resize(n); for (auto &x : len) if (!(in >> x) || x < 1) return bad("len"); }
    else if (kw == "order") { if (!(in >> n)) return bad("order"); order.resize(n); for (auto &x : order) if (!(in >> x)) return bad("order"); }
    else if (kw == "bins") {
      if (!(in >> n)) return bad("bins");
      rng.lo.resize(n); rng.hi.resize(n); rng.res.resize(n);
      for (size_t b = 0; b < n; ++b) if (!(in >> rng.lo[b] >> rng.hi[b] >> rng.res[b]) || rng.lo[b] > rng.hi[b]) return bad("bins");
    } else if (kw == "models") {
      if (!(in >> n)) return bad("models");
      pm.resize(n); model_bins.resize(n);
      for (size_t m = 0; m < n; ++m) {
        size_t nb = 0; PlanModel &x = pm[m];
        if (!(in >> x.cls >> x.per_block >> x.M >> x.fbQ >> x.vit_cls >> x.vitx_cls >> x.fb_cls >> nb) || x.per_block < 1) return bad("models");
        if (x.vit_cls < 0 || x.vit_cls >= NVC || x.vitx_cls < 0 || x.vitx_cls >= NVC || x.fb_cls < 0 || x.fb_cls >= NFC) return bad("model classes");
        model_bins[m].resize(nb); for (auto &b : model_bins[m]) if (!(in >> b)) return bad("model bins");
      }
    } else if (kw == "lane") { if (!(in >> n)) return bad("lane"); lane.resize(n); for (auto &x : lane) if (!(in >> x)) return bad("lane"); }
    else if (kw == "caps") {
      if (!(in >> cp.fwork >> cp.ework >> cp.rwork >> cp.pass >> cp.reg >> cp.events_f >> cp.events_e >> cp.seen_rwork >> cp.hens >> cp.div_cand >> cp.div_nores >> cp.div_fwork >>
            cp.div_ework >> cp.div_rwork >> cp.fl_cand >> cp.fl_nores >> cp.fl_fwork >> cp.fl_ework >> cp.fl_rwork >> cp.ws_per_cell >> cp.z1_per_pair)) return bad("caps");
    } else if (kw == "cnt") { Cnt c; if (!(in >> c.block >> c.k >> c.v) || c.k >= (uint64_t)CC_SIZE) return bad("cnt"); cnts.push_back(c); drained = true; }
    else if (kw == "tops") { if (!(in >> tops[0] >> tops[1] >> tops[2] >> tops[3])) return bad("tops"); drained = true; }
    else if (kw == "blocks") { int b = 1; if (!(in >> b)) return bad("blocks"); blocks = b != 0; }
    else return bad(kw.c_str());
  }
  // what the library guarantees the plan: ranges inside the order, sequences and bins that exist
  int maxL = 0;
  for (int32_t L : len) maxL = std::max(maxL, (int)L);
  for (uint32_t q : order) if (q >= len.size()) return bad("order entry");
  for (size_t b = 0; b < rng.lo.size(); ++b) if (rng.hi[b] > order.size()) return bad("bin range");
  for (auto &mb : model_bins) for (uint32_t b : mb) if (b >= rng.lo.size()) return bad("model bin");
  for (uint32_t m : lane) if (m >= pm.size()) return bad("lane model");
  if (has_share) opt.long_share = share.c_str();
  const uint32_t nbins = (uint32_t)rng.lo.size();
  rng.tag = 7;

  printf("{");
  // ---- the host-driven cascade: chunks of the lane's models under the pair budget, one table per chunk ----
  printf("\"host\":[");
  for (size_t i0 = 0, nchunk = 0; i0 < lane.size();) {
    const LaneModels lm = lane_models(rng, lane, model_bins, i0, opt.pair_budget);
    i0 = lm.next;
    if (lm.mws.empty() || lm.total_pairs == 0) continue;
    printf("%s{\"next\":%zu,\"total_pairs\":%" PRIu64 ",", nchunk++ ? "," : "", lm.next, lm.total_pairs);
    mws_out(lm.mws);
    key("key", plan_key_host(11, 22, opt.pair_budget, i0, rng.tag, lm.mws, model_bins));
    const BlockTable t = block_table_host(lm.mws, pm.data(), model_bins, rng, order.data(), len.data());
    table(t, t.groups, blocks);
    printf("}");
  }
  printf("],");
  // ---- the device-driven cascade ----
  const std::vector<uint64_t> no_key; const PlanGroups no_groups;
  CascadePlan pl = cascade_plan(11, 22, rng, lane, model_bins, pm.data(), order.data(), len.data(), maxL, nbins, opt, no_key, no_groups);
  printf("\"verdict\":%d,\"total_pairs\":%" PRIu64 ",", (int)pl.verdict, pl.total_pairs);
  mws_out(pl.mws);
  printf("\"nparts\":%d,\"Lcut\":%d,", pl.parts.nparts, pl.parts.Lcut);
  arr("Lcuts", pl.parts.Lcuts);
  printf("\"cut\":[");
  for (size_t k = 0; k < pl.parts.cut.size(); ++k) { printf("%s", k ? "," : ""); list(pl.parts.cut[k]); }
  printf("],");
  key("key", pl.key);
  printf("\"dev\":{"); table(pl.table, pl.groups, blocks); printf("},");
  arr("order", pl.order);
  if (pl.verdict == PLAN_GO) {
    // the key is the resident one: no table is built and the groups are the resident ones
    const CascadePlan again = cascade_plan(11, 22, rng, lane, model_bins, pm.data(), order.data(), len.data(), maxL, nbins, opt, pl.key, pl.groups);
    printf("\"resident\":%d,\"resident_blocks\":%zu,\"resident_same\":%d,", (int)again.resident, again.table.work.size(),
           (int)(again.groups == pl.groups && again.order == pl.order && again.subs.size() == pl.subs.size()));
    caps_out("caps_before", cp, ",");
    const TableSizes ts = size_tables(pl.subs, cp, pl.mws, pm.data(), model_bins, pl.total_pairs, opt.shrink, ws_budget);
    printf("\"subs\":[");
    for (size_t g = 0; g < pl.subs.size(); ++g) {
      const Sub &sb = pl.subs[g];
      std::vector<int> vit, fb;
      for (int c = 0; c < NVC; ++c) if (sb.vit[c]) vit.push_back(c);
      for (int c = 0; c < NFC; ++c) if (sb.fb[c]) fb.push_back(c);
      printf("%s{\"Q\":%d,\"maxM\":%d,\"first\":%zu,\"nblocks\":%zu,\"pairs\":%" PRIu64 ",", g ? "," : "", sb.Q, sb.maxM, sb.first, sb.nblocks, sb.pairs);
      arr("vit", vit); arr("fb", fb);
      printf("\"cap_cand\":%u,\"cap_nores\":%u,\"cap_f\":%u,\"cap_e\":%u,\"cap_r\":%u,\"o_cand\":%zu,\"o_nores\":%zu,\"o_vq\":%zu,\"o_f\":%zu,\"o_e\":%zu,\"o_r\":%zu}",
             sb.cap_cand, sb.cap_nores, sb.cap_f, sb.cap_e, sb.cap_r, sb.o_cand, sb.o_nores, sb.o_vq, sb.o_f, sb.o_e, sb.o_r);
    }
    printf("],\"tot_cand\":%zu,\"tot_nores\":%zu,\"tot_f\":%zu,\"tot_e\":%zu,\"tot_r\":%zu,\"cell_sum\":%.17g,\"ws_want\":%zu,", ts.tot_cand, ts.tot_nores, ts.tot_f, ts.tot_e, ts.tot_r,
           ts.cell_sum, ts.ws_want);
    const uint64_t z1 = zone1_floats(ws_floats, pl.total_pairs, cp);
    printf("\"z1\":%" PRIu64 ",", z1);
    caps_out("caps", cp, ",");
    if (drained) {
      std::vector<uint32_t> h_cnt((pl.subs.size() + 1) * CC_SIZE, 0);
      for (const Cnt &c : cnts) { if (c.block > pl.subs.size()) return bad("cnt block"); h_cnt[c.block * CC_SIZE + c.k] = (uint32_t)c.v; }
      const Lesson ls = learn_from(h_cnt.data(), tops, pl.subs, cp, opt.shrink, pl.total_pairs, ts.cell_sum, z1, ws_floats - z1);
      printf("\"lesson\":{\"fits\":%d,\"pairs_vit\":%" PRIu64 ",\"pairs_vit_exact\":%" PRIu64 ",\"n_cand\":%" PRIu64 ",\"n_nores\":%" PRIu64 ",\"over\":[", (int)ls.fits, ls.pairs_vit,
             ls.pairs_vit_exact, ls.n_cand, ls.n_nores);
      for (size_t i = 0; i < ls.over.size(); ++i)
        printf("%s[\"%s\",%d,%d,%" PRIu64 ",%" PRIu64 "]", i ? "," : "", ls.over[i].what, ls.over[i].group, ls.over[i].cls, ls.over[i].wanted, ls.over[i].cap);
      printf("]},");
      caps_out("caps_after", cp, ",");
    }
  }
  printf("\"end\":1}\n");
  return 0;
}
