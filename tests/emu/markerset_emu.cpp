// markerset_emu.cpp -- TEST INFRASTRUCTURE: the arithmetic, the rounds, the tile lists and the output batches of MarkerSetBuilder
// (checkm_amd/csrc/markerset_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernels' own arithmetic.
// The kernels of kernels_markerset.hip are restated as loops over their blocks, wavefronts and lanes; every buffer a kernel writes has
// exactly the size the library gives it and is reached through .at(), the tile counts start from a poison value, so that a slot beyond a
// batch or a count that was never written shows.  Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/markerset_dev.h"

using namespace ckm;

namespace {
struct Table {
  uint32_t G, C;
  const uint8_t *cls;
  std::vector<uint32_t> off;
  std::vector<int32_t> pos;
};
void make_table(uint32_t G, uint32_t C, const uint8_t *cls, const uint64_t *pos_off, const int64_t *pos, Table &T) {
  const uint64_t cells = (uint64_t)G * C;
  T.G = G; T.C = C; T.cls = cls;
  T.off.resize(cells + 1);
  for (uint64_t k = 0; k <= cells; ++k) T.off[k] = (uint32_t)pos_off[k];
  T.pos.resize(pos_off[cells]);
  for (uint64_t k = 0; k < T.pos.size(); ++k) T.pos[k] = (int32_t)pos[k];
}

struct Result {
  std::vector<uint64_t> pair_off;
  std::vector<uint32_t> pi, pj, count;
  uint64_t nbatches = 0, nrounds = 0, tests = 0;
} g_last;

// mset_pack_kernel: a thread per entry
void pack(const Table &T, const ms::Round &R, const uint32_t *qg, const uint32_t *qm, std::vector<ms::Entry> &pk) {
  pk.assign(R.entries, ms::Entry{-1, 0xFFFFFFFFu});
  const uint32_t nq = (uint32_t)R.queries.size();
  for (uint64_t e = 0; e < R.entries; ++e) {
    const ms::Query Q = R.queries[ms::find_query(nq, e, [&](uint32_t k) { return R.queries[k].pk_off; })];
    const uint64_t local = e - Q.pk_off;
    const uint32_t gi = (uint32_t)(local / Q.nm), mi = (uint32_t)(local % Q.nm);
    const uint64_t cell = (uint64_t)qg[Q.g_off + gi] * T.C + qm[Q.m_off + mi];
    const uint32_t o = T.off.at(cell), n = T.off.at(cell + 1) - o;
    pk.at(e) = ms::Entry{n ? T.pos.at(o) : 0, n};
  }
}

// mset_tile_kernel: one block
void tile_block(bool fill, const Table &T, const ms::Round &R, const ms::Tile &tile, const uint32_t *qg, const uint32_t *qm, const std::vector<ms::Entry> &pk, int32_t D,
                double thr, uint32_t row_lo, uint32_t row_hi, std::vector<uint32_t> &tile_count, const std::vector<uint64_t> &row_base,
                const std::vector<uint32_t> &row_total, uint64_t batch_base, std::vector<uint32_t> &pi, std::vector<uint32_t> &pj, std::vector<uint32_t> &pc) {
  const ms::Query Q = R.queries.at(tile.q);
  const uint32_t i0 = tile.ti * ms::TILE, j0 = tile.tj * ms::TILE, ntj = ms::tiles_for(Q.nm);
  if (fill) {
    bool any = false;
    for (uint32_t thread = 0; thread < (uint32_t)ms::TILE; ++thread) {
      const uint32_t i = i0 + thread, row = Q.row_off + i;
      if (i < Q.nm && row >= row_lo && row < row_hi) {
        (void)tile_count.at(Q.cnt_off + (uint64_t)i * ntj + (tile.tj + 1 < ntj ? tile.tj + 1 : tile.tj));      // both offsets it reads are the row's
        any |= ms::tile_pairs(&tile_count.at(Q.cnt_off + (uint64_t)i * ntj), tile.tj, ntj, row_total.at(row)) != 0;
      }
    }
    if (!any) return;
  }
  auto entry = [&](uint32_t gi, uint32_t m) { return m < Q.nm ? pk.at(Q.pk_off + (uint64_t)gi * Q.nm + m) : ms::Entry{0, 0u}; };
  for (int wave = 0; wave < ms::WAVES; ++wave)
    for (int r = 0; r < ms::ROWS_PER_WAVE; ++r) {
      const uint32_t ri = (uint32_t)(wave * ms::ROWS_PER_WAVE + r), i = i0 + ri, row = Q.row_off + i;
      uint32_t cnt[ms::WAVE];
      for (int lane = 0; lane < ms::WAVE; ++lane) {
        cnt[lane] = 0;
        const uint32_t j = j0 + (uint32_t)lane;
        for (uint32_t gi = 0; gi < Q.ng; ++gi) {
          const ms::Entry ei = entry(gi, i), ej = entry(gi, j);
          cnt[lane] += ms::pair_step(ei, ej, D, [&] {
            const uint64_t cell = (uint64_t)qg[Q.g_off + gi] * T.C;
            return ms::near_any(&T.pos.at(T.off.at(cell + qm[Q.m_off + i])), ei.n, &T.pos.at(T.off.at(cell + qm[Q.m_off + j])), ej.n, D);
          });
        }
      }
      if (i >= Q.nm || row < row_lo || row >= row_hi) continue;
      uint64_t ballot = 0;
      for (int lane = 0; lane < ms::WAVE; ++lane) {
        const uint32_t j = j0 + (uint32_t)lane;
        if (j < Q.nm && j > i && ms::reported(cnt[lane], Q.ng, thr)) ballot |= (uint64_t)1 << lane;
      }
      const uint64_t at = Q.cnt_off + (uint64_t)i * ntj + tile.tj;
      if (!fill) { tile_count.at(at) = (uint32_t)__builtin_popcountll(ballot); continue; }
      for (int lane = 0; lane < ms::WAVE; ++lane) {
        if (!(ballot >> lane & 1)) continue;
        const int below = __builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1));
        const uint64_t slot = ms::pair_slot(row_base.at(row), tile_count.at(at), below, batch_base);
        pi.at(slot) = i; pj.at(slot) = j0 + (uint32_t)lane; pc.at(slot) = cnt[lane];
      }
    }
}

// mset_scan_kernel: a wavefront per row
void scan(const ms::Round &R, std::vector<uint32_t> &tile_count, std::vector<uint32_t> &row_total) {
  const uint32_t nq = (uint32_t)R.queries.size();
  for (uint32_t k = 0; k < R.rows; ++k) {
    const ms::Query Q = R.queries[ms::find_query(nq, k, [&](uint32_t q) { return (uint64_t)R.queries[q].row_off; })];
    const uint32_t i = k - Q.row_off, ntj = ms::tiles_for(Q.nm);
    (void)tile_count.at(Q.cnt_off + (uint64_t)i * ntj + ntj - 1);                          // the whole row lies in the buffer
    row_total.at(k) = pc::row_scan_host(&tile_count.at(Q.cnt_off + (uint64_t)i * ntj), 1, i / ms::TILE, ntj);
  }
}
}  // namespace

// ckm_mset_check: 0, 1 (bad argument) or 2 (size limit)
extern "C" int emu_mset_check(uint32_t G, uint32_t C, const uint8_t *cls, const uint64_t *pos_off, const int64_t *pos, uint32_t nq, const uint64_t *qg_off, const uint32_t *qg,
                              const uint64_t *qm_off, const uint32_t *qm, double dist) {
  std::string why;
  int kind = ms::check_dist(dist, why);
  if (kind == ms::ARGS_OK) kind = ms::check_table(G, C, cls, pos_off, pos, why);
  if (kind == ms::ARGS_OK && (nq || qg_off)) kind = ms::check_queries(G, C, nq, qg_off, qg, qm_off, qm, why);
  return kind;
}

// ckm_mset_markers on the host: flag [nq * C]; counts [nq * C * 3] or NULL
extern "C" int emu_mset_markers(uint32_t G, uint32_t C, const uint8_t *cls, const uint64_t *pos_off, const int64_t *pos, uint32_t nq, const uint64_t *qg_off, const uint32_t *qg,
                                const double *tU, const double *tS, uint8_t *flag, uint32_t *counts) {
  std::string why;
  int kind = ms::check_table(G, C, cls, pos_off, pos, why);
  if (kind == ms::ARGS_OK) kind = ms::check_queries(G, C, nq, qg_off, qg, nullptr, nullptr, why);
  if (kind != ms::ARGS_OK) return kind;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t block = 0; block * (uint32_t)ms::THREADS < C; ++block)
      for (uint32_t thread = 0; thread < (uint32_t)ms::THREADS; ++thread) {
        const uint32_t f = block * ms::THREADS + thread;
        if (f >= C) continue;
        const uint64_t g0 = qg_off[q], ng = qg_off[q + 1] - g0;
        uint32_t ub = 0, single = 0, dup = 0;
        for (uint64_t k = 0; k < ng; ++k) ms::class_step(cls[(uint64_t)qg[g0 + k] * C + f], ub, single, dup);
        const uint64_t at = (uint64_t)q * C + f;
        flag[at] = ms::family_flags(ub, single, dup, (uint32_t)ng, tU[q], tS[q]);
        if (counts) { counts[at * 3] = ub; counts[at * 3 + 1] = single; counts[at * 3 + 2] = dup; }
      }
  return 0;
}

// ckm_mset_colocated on the host; the result stays here until emu_mset_fetch.  info: npairs, batches, rounds, tests
extern "C" int emu_mset_colocated(uint32_t G, uint32_t C, const uint8_t *cls, const uint64_t *pos_off, const int64_t *pos, uint32_t nq, const uint64_t *qg_off,
                                  const uint32_t *qg, const uint64_t *qm_off, const uint32_t *qm, double dist, double thr, uint64_t budget_bytes, uint64_t *info) {
  std::string why;
  int kind = ms::check_dist(dist, why);
  if (kind == ms::ARGS_OK) kind = ms::check_table(G, C, cls, pos_off, pos, why);
  if (kind == ms::ARGS_OK) kind = qm_off ? ms::check_queries(G, C, nq, qg_off, qg, qm_off, qm, why) : (int)ms::ARGS_INVALID;
  if (kind != ms::ARGS_OK || !budget_bytes) return kind ? kind : 1;
  Table T;
  make_table(G, C, cls, pos_off, pos, T);
  const int32_t D = (int32_t)dist;
  const uint64_t cap = ms::budget_pairs(budget_bytes);
  Result o;
  o.pair_off.assign((size_t)nq + 1, 0);
  for (uint32_t q = 0; q < nq; ++q) {
    const uint64_t ng = qg_off[q + 1] - qg_off[q], nm = qm_off[q + 1] - qm_off[q];
    o.tests += nm ? ng * (nm * (nm - 1) / 2) : 0;
  }
  ms::Round R;
  std::vector<ms::Entry> pk;
  std::vector<uint32_t> tile_count, row_total, pi, pj, pc;
  std::vector<uint64_t> row_base;
  std::vector<ms::Group> groups;
  for (uint32_t q0 = 0; q0 < nq;) {
    const uint32_t q1 = ms::next_round(nq, qg_off, qm_off, budget_bytes, q0);
    if (q1 <= q0) return 3;
    ms::build_round(qg_off, qm_off, q0, q1, R);
    for (uint32_t q = q0; q < q1; ++q) o.pair_off[q + 1] = o.pair_off[q];
    if (!R.tiles.empty()) {
      o.nrounds += 1;
      pack(T, R, qg, qm, pk);
      tile_count.assign(R.counts, 0xDEADBEEFu); row_total.assign(R.rows, 0xDEADBEEFu); row_base.assign(R.rows, 0);
      for (const ms::Tile &t : R.tiles) tile_block(false, T, R, t, qg, qm, pk, D, thr, 0, R.rows, tile_count, row_base, row_total, 0, pi, pj, pc);
      scan(R, tile_count, row_total);
      const uint64_t run = pc::row_prefix(row_total.data(), R.rows, row_base.data());
      for (uint32_t q = q0; q < q1; ++q) {
        const ms::Query &Q = R.queries[q - q0];
        uint64_t n = 0;
        for (uint32_t k = 0; k < Q.nrows; ++k) n += row_total[Q.row_off + k];
        o.pair_off[q + 1] = o.pair_off[q] + n;
      }
      groups.clear();
      ms::plan_groups(row_total.data(), R.rows, cap, R.tiles, groups);
      uint64_t seen = 0;
      for (const ms::Group &g : groups) {
        if (g.base != seen || g.t_lo > g.t_hi || g.t_hi > R.tiles.size()) return 4;
        pi.assign(g.npairs, 0xFFFFFFFFu); pj.assign(g.npairs, 0xFFFFFFFFu); pc.assign(g.npairs, 0xFFFFFFFFu);
        for (uint32_t t = g.t_lo; t < g.t_hi; ++t) tile_block(true, T, R, R.tiles[t], qg, qm, pk, D, thr, g.row_lo, g.row_hi, tile_count, row_base, row_total, g.base, pi, pj, pc);
        // the tiles outside [t_lo, t_hi) hold no row of the batch
        for (uint32_t t = 0; t < R.tiles.size(); ++t)
          if ((t < g.t_lo || t >= g.t_hi) && R.tiles[t].row0 < g.row_hi && (uint64_t)R.tiles[t].row0 + ms::TILE > g.row_lo) return 5;
        for (uint64_t k = 0; k < g.npairs; ++k) if (pi[k] == 0xFFFFFFFFu) return 6;             // every slot of the batch was written
        o.pi.insert(o.pi.end(), pi.begin(), pi.end()); o.pj.insert(o.pj.end(), pj.begin(), pj.end()); o.count.insert(o.count.end(), pc.begin(), pc.end());
        o.nbatches += 1; seen += g.npairs;
      }
      if (seen != run) return 7;
    }
    q0 = q1;
  }
  info[0] = o.pi.size(); info[1] = o.nbatches; info[2] = o.nrounds; info[3] = o.tests;
  g_last = std::move(o);
  return 0;
}

extern "C" void emu_mset_fetch(uint64_t *pair_off, uint32_t *pi, uint32_t *pj, uint32_t *count) {
  memcpy(pair_off, g_last.pair_off.data(), g_last.pair_off.size() * 8);
  if (!g_last.pi.empty()) {
    memcpy(pi, g_last.pi.data(), g_last.pi.size() * 4); memcpy(pj, g_last.pj.data(), g_last.pj.size() * 4); memcpy(count, g_last.count.data(), g_last.count.size() * 4);
  }
}
