// placement_host_check.cpp -- TEST INFRASTRUCTURE: the host code of the phylogenetic placement (ckm_place_check in place_host.cpp; the
// tests, the level schedule, the chunk cuts and the arithmetic of place_dev.h, walked by its host executor through
// tests/emu/placement_emu.cpp, which this file includes) built with -fsanitize=address,undefined on the CPU.
//   <call file> <budget bytes> <damaged calls>
// The file holds whitespace-separated numbers, doubles as hexadecimal floats: N nchild S nrows nq R F G K; N + 1 child offsets; the
// children; N lengths; nrows + 1 row offsets; nrows * S row bytes; nq + 1 query offsets; nq * S query bytes; R weights; U; Uinv; pi;
// exp_len; exp_half; exp_dist; exp_pend.  Prints "check rc=<code>", one line "<query> <slot> <edge> <scan m as %a> <scan e> <ref m> <ref e>
// <f> <g>" per kept placement and "chunks <n>"; then, <damaged calls> times, the call with entries overwritten is checked
// ("damaged rc=<code>") and, where the check passes, walked as well.  Every array has exactly its stated size.
#include <cinttypes>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "../emu/placement_emu.cpp"

namespace ckm { static std::string g_last_error; void set_last_error(const std::string &m) { g_last_error = m; } }

struct Call {
  std::vector<uint64_t> child_off, row_off, q_off;
  std::vector<uint32_t> child;
  std::vector<uint8_t> rows, queries;
  std::vector<double> length, weights, U, Uinv, pi, exp_len, exp_half, exp_dist, exp_pend;
  uint32_t S = 0, R = 0, F = 0, G = 0, K = 0;
  ckm_place_args args() const {
    ckm_place_args a;
    a.nnodes = (uint32_t)child_off.size() - 1; a.child_off = child_off.data(); a.child = child.data(); a.nchild = child.size(); a.length = length.data();
    a.nsites = S; a.nrows = (uint32_t)row_off.size() - 1; a.row_off = row_off.data(); a.rows = rows.data(); a.nrow_bytes = rows.size();
    a.nqueries = (uint32_t)q_off.size() - 1; a.q_off = q_off.data(); a.queries = queries.data(); a.nquery_bytes = queries.size();
    a.nrates = R; a.weights = weights.data(); a.U = U.data(); a.Uinv = Uinv.data(); a.pi = pi.data(); a.exp_len = exp_len.data(); a.exp_half = exp_half.data();
    a.nfrac = F; a.exp_dist = exp_dist.data(); a.npend = G; a.exp_pend = exp_pend.data(); a.max_pitches = K;
    return a;
  }
};

static void walk(const Call &c, uint64_t budget, bool print) {
  const ckm_place_args a = c.args();
  const size_t n = (size_t)a.nqueries * a.max_pitches;
  std::vector<int32_t> top(n), rf(n), rg(n);
  std::vector<double> sm(n), rm(n);
  std::vector<int64_t> se(n), re(n);
  const ckm_place_out o = {top.data(), sm.data(), se.data(), rm.data(), re.data(), rf.data(), rg.data()};
  uint64_t info[2] = {0, 0};
  const int rc = emu_place_run(&a, budget, &o, info);
  if (rc) { printf("walk failed %d\n", rc); exit(5); }
  for (uint32_t q = 0; q < a.nqueries; ++q)
    for (uint32_t k = 0; k < a.max_pitches; ++k) {
      const size_t at = (size_t)q * a.max_pitches + k;
      if (top[at] < 0) continue;
      if ((uint32_t)top[at] >= a.nnodes || rf[at] < 0 || (uint32_t)rf[at] >= a.nfrac || rg[at] < 0 || (uint32_t)rg[at] >= a.npend) { printf("a result out of range\n"); exit(6); }
      if (print) printf("%u %u %d %a %" PRId64 " %a %" PRId64 " %d %d\n", q, k, top[at], sm[at], se[at], rm[at], re[at], rf[at], rg[at]);
    }
  if (print) printf("chunks %" PRIu64 "\n", info[0]);
}

template <class T, class Read>
static bool read_n(FILE *f, std::vector<T> &v, size_t n, Read &&read) {
  v.resize(n);
  for (size_t k = 0; k < n; ++k)
    if (!read(f, v[k])) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <call file> <budget bytes> <damaged calls>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Call c;
  unsigned N = 0, nchild = 0, nrows = 0, nq = 0;
  auto u64 = [](FILE *g, uint64_t &x) { return fscanf(g, "%" SCNu64, &x) == 1; };
  auto u32 = [](FILE *g, uint32_t &x) { return fscanf(g, "%" SCNu32, &x) == 1; };
  auto u8 = [](FILE *g, uint8_t &x) { unsigned v = 0; const bool ok = fscanf(g, "%u", &v) == 1 && v < 256; x = (uint8_t)v; return ok; };
  auto f64 = [](FILE *g, double &x) { return fscanf(g, "%la", &x) == 1; };
  bool ok = fscanf(f, "%u %u %u %u %u %u %u %u %u", &N, &nchild, &c.S, &nrows, &nq, &c.R, &c.F, &c.G, &c.K) == 9;
  const unsigned cap = 1u << 12;
  ok = ok && N < cap && nchild < cap && c.S < cap && nrows < cap && nq < cap && c.R < 64 && c.F < 64 && c.G < 64 && c.K < cap;
  ok = ok && read_n(f, c.child_off, (size_t)N + 1, u64) && read_n(f, c.child, nchild, u32) && read_n(f, c.length, N, f64) && read_n(f, c.row_off, (size_t)nrows + 1, u64) &&
       read_n(f, c.rows, (size_t)nrows * c.S, u8) && read_n(f, c.q_off, (size_t)nq + 1, u64) && read_n(f, c.queries, (size_t)nq * c.S, u8) && read_n(f, c.weights, c.R, f64) &&
       read_n(f, c.U, 400, f64) && read_n(f, c.Uinv, 400, f64) && read_n(f, c.pi, 20, f64) && read_n(f, c.exp_len, (size_t)N * c.R * 20, f64) &&
       read_n(f, c.exp_half, (size_t)N * c.R * 20, f64) && read_n(f, c.exp_dist, (size_t)N * c.F * 2 * c.R * 20, f64) && read_n(f, c.exp_pend, ((size_t)c.G + 1) * c.R * 20, f64);
  fclose(f);
  if (!ok) { fprintf(stderr, "malformed call file\n"); return 2; }
  const uint64_t budget = strtoull(argv[2], nullptr, 10);
  ckm_place_args a = c.args();
  const int rc = ckm_place_check(&a);
  printf("check rc=%d\n", rc);
  if (rc) printf("error: %s\n", ckm::g_last_error.c_str());
  else walk(c, budget, true);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  auto hit_offsets = [&](std::vector<uint64_t> &t) { t[rnd() % t.size()] = rnd() % 4 == 0 ? rnd() : rnd() % (t.back() + 3); };
  auto hit_doubles = [&](std::vector<double> &t) {
    const double bad[] = {-1.0, 0.0, HUGE_VAL, -HUGE_VAL, 1.0, 4.9e-324, 0.5};
    if (!t.empty()) t[rnd() % t.size()] = rnd() % 8 == 0 ? std::nan("") : bad[rnd() % 7];
  };
  for (int k = 0, n = atoi(argv[3]); k < n; ++k) {
    Call d = c;
    for (int hits = 1 + k % 3; hits > 0; --hits)
      switch (rnd() % 10) {
        case 0: hit_offsets(d.child_off); break;
        case 1: hit_offsets(d.row_off); break;
        case 2: hit_offsets(d.q_off); break;
        case 3: case 4: d.child[rnd() % d.child.size()] = (uint32_t)(rnd() % 3 ? rnd() % (d.child_off.size() + 1) : rnd()); break;
        case 5: hit_doubles(d.length); break;
        case 6: hit_doubles(rnd() % 2 ? d.exp_len : d.exp_dist); break;
        case 7: hit_doubles(rnd() % 2 ? d.weights : d.U); break;
        case 8: if (!d.queries.empty()) d.queries[rnd() % d.queries.size()] = (uint8_t)rnd(); break;
        default: d.K = (uint32_t)(rnd() % 3 ? rnd() % 8 : rnd()); d.R = rnd() % 4 ? d.R : (uint32_t)(rnd() % 12); break;
      }
    if (d.R > c.R) d.R = d.R > 8 ? 9 : c.R;        // more rates than the arrays hold only where the count alone refuses the call
    a = d.args();
    const int drc = ckm_place_check(&a);
    printf("damaged rc=%d\n", drc);
    if (!drc) walk(d, budget, false);
  }
  return 0;
}
