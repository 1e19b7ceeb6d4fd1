// genetrees_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the gene-tree tests (ckm_genetree_check and ckm_genetree_host in
// genetree_host.cpp; the checks, the walks, the quotients and the round cuts of genetree_dev.h) built with -fsanitize=address,undefined
// on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers: ntrees, then node_off, leaf_off, group_off [ntrees + 1], class_off [3 ntrees + 1],
// gpair_off [groups + 1], then per node first, last, parent, internal and length (as %a), per leaf genome, species and the three class
// rows, per class its total, per pair a and b.  Prints "check rc=<code>", one line "c <class> <double as %a>" per class, "p <pair>
// <flag>" per pair, "g <group> <node> <mixed>" per group and "rounds <n>"; then, <damaged calls> times, the call with entries of the
// node, leaf, class and pair arrays overwritten (ranges outside the tree, parents behind their children, class indices beyond the count,
// pairs beyond the tree, lengths that are not finite) is checked ("damaged rc=<code>") and, where the check passes, run as well.  Every
// array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  uint32_t T = 0;
  std::vector<uint32_t> node_off, leaf_off, group_off, class_off, gpair_off, first, last, parent, genome, species, cls, total, pa, pb;
  std::vector<uint8_t> internal;
  std::vector<double> length;
  ckm_genetree_args args() const {
    ckm_genetree_args a = {};
    a.ntrees = T; a.node_off = node_off.data(); a.leaf_off = leaf_off.data(); a.class_off = class_off.data(); a.group_off = group_off.data(); a.gpair_off = gpair_off.data();
    a.first = first.data(); a.last = last.data(); a.parent = parent.data(); a.length = length.data(); a.internal = internal.data();
    a.leaf_genome = genome.data(); a.leaf_species = species.data(); a.leaf_class = cls.data(); a.class_total = total.data(); a.pair_a = pa.data(); a.pair_b = pb.data();
    return a;
  }
};

static void walk(const Call &c, uint64_t budget, bool print) {
  const ckm_genetree_args a = c.args();
  std::vector<double> cons(c.total.size(), -1.0);
  std::vector<uint8_t> flag(c.pa.size(), 9), mixed(c.gpair_off.size() - 1, 9);
  std::vector<uint32_t> node(c.gpair_off.size() - 1, 7);
  ckm_genetree_out o = {cons.data(), flag.data(), node.data(), mixed.data()};
  ckm_genetree_info info;
  const int rc = ckm_genetree_host(&a, budget, &o, &info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  for (size_t k = 0; k < cons.size(); ++k) {
    if (!(cons[k] >= 0.0 && cons[k] <= 1.0)) { printf("a consistency that was never written\n"); exit(6); }
    if (print) printf("c %zu %a\n", k, cons[k]);
  }
  for (size_t k = 0; k < flag.size(); ++k) {
    if (flag[k] > 1) { printf("a flag that was never written\n"); exit(6); }
    if (print) printf("p %zu %u\n", k, flag[k]);
  }
  for (size_t k = 0; k < node.size(); ++k) {
    if (mixed[k] > 1) { printf("a group that was never written\n"); exit(6); }
    if (print) printf("g %zu %u %u\n", k, node[k], mixed[k]);
  }
  if (print) printf("rounds %" PRIu64 "\n", (uint64_t)info.nrounds);
}

static bool read_u32(FILE *f, std::vector<uint32_t> &v, size_t n) {
  v.resize(n);
  for (auto &x : v) if (fscanf(f, "%" SCNu32, &x) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  const size_t cap = 1u << 22;
  bool ok = fscanf(f, "%u", &c.T) == 1 && c.T < cap;
  ok = ok && read_u32(f, c.node_off, c.T + 1) && read_u32(f, c.leaf_off, c.T + 1) && read_u32(f, c.group_off, c.T + 1) && read_u32(f, c.class_off, 3 * (size_t)c.T + 1);
  ok = ok && c.group_off[c.T] < cap && read_u32(f, c.gpair_off, (size_t)c.group_off[c.T] + 1);
  ok = ok && c.node_off[c.T] < cap && c.leaf_off[c.T] < cap && c.class_off[3 * (size_t)c.T] < cap && c.gpair_off[c.group_off[c.T]] < cap;
  if (ok) {
    const size_t NN = c.node_off[c.T], NL = c.leaf_off[c.T], NC = c.class_off[3 * (size_t)c.T], NP = c.gpair_off[c.group_off[c.T]];
    std::vector<uint32_t> internal;
    ok = read_u32(f, c.first, NN) && read_u32(f, c.last, NN) && read_u32(f, c.parent, NN) && read_u32(f, internal, NN);
    c.internal.assign(internal.begin(), internal.end());
    c.length.resize(NN);
    for (auto &x : c.length) ok = ok && fscanf(f, "%la", &x) == 1;
    ok = ok && read_u32(f, c.genome, NL) && read_u32(f, c.species, NL) && read_u32(f, c.cls, 3 * NL) && read_u32(f, c.total, NC) && read_u32(f, c.pa, NP) && read_u32(f, c.pb, NP);
  }
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_genetree_args a = c.args();
  const int rc = ckm_genetree_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto hit = [&](std::vector<uint32_t> &v, uint32_t small) { if (!v.empty()) v[rnd() % v.size()] = (uint32_t)(rnd() % 4 ? rnd() % (small + 2) : rnd()); };
  static const double lengths[] = {-1.0, 0.0, 0.5, 1e300, 1.0 / 0.0, -1.0 / 0.0, 0.0 / 0.0};
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 10) {
        case 0: hit(d.first, 40); break;
        case 1: hit(d.last, 40); break;                                           // ranges outside the tree
        case 2: hit(d.parent, 60); break;                                         // a parent behind its child
        case 3: if (!d.internal.empty()) d.internal[rnd() % d.internal.size()] = (uint8_t)(rnd() % 3); break;
        case 4: if (!d.length.empty()) d.length[rnd() % d.length.size()] = lengths[rnd() % 7]; break;
        case 5: hit(d.cls, 6); break;                                             // a class index beyond the class count
        case 6: hit(d.total, 6); break;
        case 7: hit(d.pa, 40); break;
        case 8: hit(d.pb, 40); break;                                             // a pair that names a leaf beyond the tree
        default: hit(d.species, 3); break;                                        // (any value is a species: the call runs)
      }
    a = d.args();
    const int drc = ckm_genetree_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
