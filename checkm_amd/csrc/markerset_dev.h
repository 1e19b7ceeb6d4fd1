// markerset_dev.h -- the arithmetic and the host-side geometry of MarkerSetBuilder (scripts/genometreeworkflow/markerSetBuilder.py of the
// reference: markerGenes :131-157, colocatedGenes :159-192, missingGenes :486-510, duplicateGenes :512-536), written once for the kernels
// (kernels_markerset.hip) and for the host executor of the CPU tests (tests/emu/markerset_emu.cpp).
//
// The resident table, for C families and G genomes:
//   cls[g * C + f]       the count class of family f in genome g: 0, 1 or 2 ("more than one"); genome-major, so the lanes that own
//                        neighbouring families read neighbouring bytes
//   pos_off[g * C + f]   first entry of the start positions of the copies of f in g; pos_off[G * C] = all positions
//   pos[..]              int32 start positions, contigs laid end to end as IMG._genomeFamilyPositions lays them, every one in [0, 2^31)
// The count class and the copies are independent: a family is counted from the annotation table, a copy needs a GFF record.
//
// Marker pass: a lane owns a family of a query, walks the query's genomes and keeps three counts; the reference's tests are
//   (double)ubiquity >= tU && (double)single >= tS,   (double)(n - ubiquity) >= tU,   (double)duplicate >= tU
// (an int against the float the caller computed; the counts are far below 2^53, so the conversion is exact).
//
// Co-location pass: a query is a genome list and a marker list.  Its (genome, marker) entries are packed densely as (first copy, copies);
// copies beyond the first stay in the table's own list, which is the overflow list of every query.  A lane owns a pair (i, j), i < j, of
// the marker list and counts the genomes in which both markers have a copy and some pair of copies has |start1 - start2| < D.  After the
// last genome: (double)count / (double)nGenomes > genomeThreshold, one IEEE division (the library is built with -ffp-contract=off).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "pairs_dev.h"
#include "wave_const.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MS_HD __host__ __device__ __forceinline__
#else
#define MS_HD inline
#endif

namespace ckm {
namespace ms {

using ckm::WAVE;
constexpr int TILE = WAVE;                         // rows and columns of a tile of marker pairs: a lane per column
constexpr int WAVES = 4;                           // wavefronts of a block
constexpr int ROWS_PER_WAVE = TILE / WAVES;        // rows one wavefront walks: their counts live in registers
constexpr int GCHUNK = 16;                         // genomes of a query staged in LDS at once
constexpr int THREADS = WAVE * WAVES;
constexpr uint32_t MAX_GENOMES = 1u << 24;         // G, and the genomes of a query: counts stay exact in uint32 and in float64
constexpr uint32_t MAX_FAMILIES = 1u << 24;        // C
constexpr uint32_t MAX_MARKERS = 1u << 20;         // markers of one query
constexpr uint64_t MAX_POSITIONS = 0x7fffffffull;  // entries of pos: pos_off travels as uint32
constexpr uint64_t MAX_CELLS = 1ull << 40;         // G * C
constexpr uint32_t PAIR_BYTES = 12;                // a reported pair: i, j, count
constexpr uint8_t FLAG_MARKER = 1, FLAG_MISSING = 2, FLAG_DUPLICATE = 4;

struct Entry { int32_t first; uint32_t n; };       // a (genome, marker) of a query: start of the first copy, copies

// What the kernels know of a query of one round.  A query without a pair to test (no genome, fewer than two markers) has no rows.
struct Query {
  uint64_t g_off, m_off;      // its genomes and markers in the call's lists
  uint64_t pk_off;            // its packed entries [ng][nm], in the round's buffer
  uint64_t cnt_off;           // its tile counts [nm][ntiles], in the round's buffer
  uint32_t row_off;           // rows of the queries of the round in front of it
  uint32_t ng, nm, nrows;     // nrows = nm, or 0
};
struct Tile { uint32_t q, ti, tj, row0; };         // query of the round, tile row and column (tj >= ti), row0 = row_off + ti * TILE

MS_HD uint32_t tiles_for(uint32_t nm) { return (nm + (uint32_t)TILE - 1) / (uint32_t)TILE; }

// what the kernels take by value (kernels_markerset.hip, ckm_markerset.hip)
struct MsetTableDev {
  const uint8_t *cls;          // [G * C]
  const uint32_t *pos_off;     // [G * C + 1]
  const int32_t *pos;
  uint32_t G, C;
};

struct MsetOut {
  const uint64_t *row_base;    // [rows of the round]: reported pairs of the rows before
  const uint32_t *row_total;   // [rows of the round]: reported pairs of the row
  uint64_t batch_base, cap;    // first pair of this output batch; pairs the columns hold
  uint32_t *pi, *pj, *count;   // [cap]
};

// ---- marker pass --------------------------------------------------------------------------------------------------------------------------
MS_HD void class_step(uint32_t c, uint32_t &ubiquity, uint32_t &single, uint32_t &duplicate) {
  ubiquity += c > 0 ? 1u : 0u;
  single += c == 1 ? 1u : 0u;
  duplicate += c > 1 ? 1u : 0u;
}
MS_HD uint8_t family_flags(uint32_t ubiquity, uint32_t single, uint32_t duplicate, uint32_t ngenomes, double tU, double tS) {
  uint8_t f = 0;
  if ((double)ubiquity >= tU && (double)single >= tS) f |= FLAG_MARKER;
  if ((double)(ngenomes - ubiquity) >= tU) f |= FLAG_MISSING;
  if ((double)duplicate >= tU) f |= FLAG_DUPLICATE;
  return f;
}

// ---- co-location pass ---------------------------------------------------------------------------------------------------------------------
// both starts in [0, 2^31): the difference cannot overflow
MS_HD bool near(int32_t a, int32_t b, int32_t D) { const int32_t d = a - b; return (d < 0 ? -d : d) < D; }

// the multi-copy case, exactly: any pair of copies
MS_HD bool near_any(const int32_t *a, uint32_t na, const int32_t *b, uint32_t nb, int32_t D) {
  for (uint32_t x = 0; x < na; ++x)
    for (uint32_t y = 0; y < nb; ++y)
      if (near(a[x], b[y], D)) return true;
  return false;
}

// one genome of one pair; walk() is called only when both markers are present and one of them has more than one copy
template <class Walk>
MS_HD uint32_t pair_step(const Entry &a, const Entry &b, int32_t D, Walk &&walk) {
  if (a.n == 0 || b.n == 0) return 0u;
  if (a.n == 1 && b.n == 1) return near(a.first, b.first, D) ? 1u : 0u;
  return walk() ? 1u : 0u;
}

// colocatedGenes :189, in its order
MS_HD bool reported(uint32_t count, uint32_t ngenomes, double genome_threshold) {
  if (ngenomes == 0) return false;                 // the reference never gets here without a genome
  return (double)count / (double)ngenomes > genome_threshold;
}

// Where the fill pass puts a reported pair, and what a row reports in a tile column after the scan (the fill pass skips a tile none of
// whose rows reports anything): pairs_dev.h
using pc::pair_slot;
using pc::tile_pairs;

// the last query q of [0, n) with key(q) <= x; key never falls and key(0) <= x.  Queries without entries repeat their neighbour's key and
// are never the answer for an x that belongs to somebody.
template <class Key>
MS_HD uint32_t find_query(uint32_t n, uint64_t x, Key &&key) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

// the distance threshold as the kernels take it
inline int check_dist(double dist_threshold, std::string &why) {
  if (!(dist_threshold == dist_threshold) || std::floor(dist_threshold) != dist_threshold) { why = "distThreshold is not an integer"; return ARGS_INVALID; }
  if (dist_threshold < 0.0 || dist_threshold > 2147483647.0) { why = "distThreshold does not fit int32"; return ARGS_RANGE; }
  return ARGS_OK;
}

// The table as the caller holds it: positions are int64 there, and one that does not fit int32 (or is negative) is refused.  No entry of
// pos is read before pos_off is known to be in order.
inline int check_table(uint32_t G, uint32_t C, const uint8_t *cls, const uint64_t *pos_off, const int64_t *pos, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (G > MAX_GENOMES) return no(ARGS_RANGE, "more than 2^24 genomes");
  if (C > MAX_FAMILIES) return no(ARGS_RANGE, "more than 2^24 families");
  const uint64_t cells = (uint64_t)G * C;
  if (cells > MAX_CELLS) return no(ARGS_RANGE, "more than 2^40 (genome, family) cells");
  if (!pos_off || (cells && !cls)) return no(ARGS_INVALID, "NULL argument");
  if (pos_off[0] != 0) return no(ARGS_INVALID, "pos_off does not start at 0");
  for (uint64_t k = 0; k < cells; ++k) {
    if (pos_off[k + 1] < pos_off[k]) return no(ARGS_INVALID, "pos_off falls at cell " + std::to_string(k));
    if (cls[k] > 2) return no(ARGS_INVALID, "count class " + std::to_string(cls[k]) + " at cell " + std::to_string(k));
  }
  const uint64_t npos = pos_off[cells];
  if (npos > MAX_POSITIONS) return no(ARGS_RANGE, "more than 2^31 - 1 positions");
  if (npos && !pos) return no(ARGS_INVALID, "NULL positions");
  for (uint64_t k = 0; k < npos; ++k)
    if (pos[k] < 0 || pos[k] > 2147483647ll) return no(ARGS_RANGE, "position " + std::to_string(pos[k]) + " does not fit int32");
  return ARGS_OK;
}

// The queries of a call: qg_off[nq + 1] into qg (genome indices), and for the co-location pass qm_off[nq + 1] into qm (family indices);
// qm_off may be NULL (marker pass).
inline int check_queries(uint32_t G, uint32_t C, uint32_t nq, const uint64_t *qg_off, const uint32_t *qg, const uint64_t *qm_off, const uint32_t *qm, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (!qg_off) return no(ARGS_INVALID, "NULL argument");
  if (qg_off[0] != 0) return no(ARGS_INVALID, "qg_off does not start at 0");
  for (uint32_t q = 0; q < nq; ++q) {
    if (qg_off[q + 1] < qg_off[q]) return no(ARGS_INVALID, "qg_off falls at query " + std::to_string(q));
    if (qg_off[q + 1] - qg_off[q] > MAX_GENOMES) return no(ARGS_RANGE, "more than 2^24 genomes in query " + std::to_string(q));
  }
  if (qg_off[nq] && !qg) return no(ARGS_INVALID, "NULL genome list");
  for (uint64_t k = 0; k < qg_off[nq]; ++k)
    if (qg[k] >= G) return no(ARGS_INVALID, "genome index " + std::to_string(qg[k]) + " beyond the table");
  if (!qm_off) return ARGS_OK;
  if (qm_off[0] != 0) return no(ARGS_INVALID, "qm_off does not start at 0");
  for (uint32_t q = 0; q < nq; ++q) {
    if (qm_off[q + 1] < qm_off[q]) return no(ARGS_INVALID, "qm_off falls at query " + std::to_string(q));
    if (qm_off[q + 1] - qm_off[q] > MAX_MARKERS) return no(ARGS_RANGE, "more than 2^20 markers in query " + std::to_string(q));
  }
  if (qm_off[nq] && !qm) return no(ARGS_INVALID, "NULL marker list");
  for (uint64_t k = 0; k < qm_off[nq]; ++k)
    if (qm[k] >= C) return no(ARGS_INVALID, "family index " + std::to_string(qm[k]) + " beyond the table");
  return ARGS_OK;
}

// what one query needs on the device during a round
inline uint64_t query_entries(uint64_t ng, uint64_t nm) { return ng && nm > 1 ? ng * nm : 0; }
inline uint64_t query_counts(uint64_t ng, uint64_t nm) { return ng && nm > 1 ? nm * tiles_for((uint32_t)nm) : 0; }
inline uint64_t query_tiles(uint64_t ng, uint64_t nm) { const uint64_t t = tiles_for((uint32_t)nm); return ng && nm > 1 ? t * (t + 1) / 2 : 0; }
inline uint64_t query_bytes(uint64_t ng, uint64_t nm) {
  return query_entries(ng, nm) * sizeof(Entry) + query_counts(ng, nm) * 4 + query_tiles(ng, nm) * sizeof(Tile) + (ng && nm > 1 ? nm * 12 : 0);
}

// A round: queries [q0, q1) whose packed entries, tile counts, tile list and row tables fit budget_bytes -- always at least one query,
// never 2^31 rows or tiles.  Returns q1.
inline uint32_t next_round(uint32_t nq, const uint64_t *qg_off, const uint64_t *qm_off, uint64_t budget_bytes, uint32_t q0) {
  uint64_t bytes = 0, rows = 0, tiles = 0;
  uint32_t q = q0;
  for (; q < nq; ++q) {
    const uint64_t ng = qg_off[q + 1] - qg_off[q], nm = qm_off[q + 1] - qm_off[q];
    const uint64_t b = query_bytes(ng, nm), r = ng && nm > 1 ? nm : 0, t = query_tiles(ng, nm);
    if (q > q0 && (bytes + b > budget_bytes || rows + r > 0x7fffffffull || tiles + t > 0x7fffffffull)) break;
    bytes += b; rows += r; tiles += t;
  }
  return q;
}

// The descriptors and the tile list of a round: the tiles of all its queries as ONE list, in (query, tile row, tile column) order, so
// that row0 never falls along the list.
struct Round {
  std::vector<Query> queries;
  std::vector<Tile> tiles;
  uint64_t entries = 0, counts = 0;
  uint32_t rows = 0;
};
inline void build_round(const uint64_t *qg_off, const uint64_t *qm_off, uint32_t q0, uint32_t q1, Round &R) {
  R.queries.clear(); R.tiles.clear(); R.entries = R.counts = 0; R.rows = 0;
  for (uint32_t q = q0; q < q1; ++q) {
    const uint64_t ng = qg_off[q + 1] - qg_off[q], nm = qm_off[q + 1] - qm_off[q];
    Query Q = {qg_off[q], qm_off[q], R.entries, R.counts, R.rows, (uint32_t)ng, (uint32_t)nm, ng && nm > 1 ? (uint32_t)nm : 0u};
    R.entries += query_entries(ng, nm); R.counts += query_counts(ng, nm); R.rows += Q.nrows;
    if (Q.nrows) {
      const uint32_t nt = tiles_for(Q.nm);
      for (uint32_t ti = 0; ti < nt; ++ti)
        for (uint32_t tj = ti; tj < nt; ++tj) R.tiles.push_back(Tile{q - q0, ti, tj, Q.row_off + ti * (uint32_t)TILE});
    }
    R.queries.push_back(Q);
  }
}

inline uint64_t budget_pairs(uint64_t budget_bytes) { return pc::budget_pairs(budget_bytes, PAIR_BYTES); }

// The tiles [t_lo, t_hi) of the round's list that hold the rows of an output batch (pairs_dev.h; the rows of a round are the rows of its
// count pass).  row0 never falls along the list: the tiles with a row in [row_lo, row_hi) are one stretch of it.
struct TileRange { uint32_t t_lo, t_hi; };
inline TileRange tile_range(const pc::Group &g, const std::vector<Tile> &tiles) {
  const auto lo = std::partition_point(tiles.begin(), tiles.end(), [&](const Tile &t) { return (uint64_t)t.row0 + TILE <= g.row_lo; });
  const auto hi = std::partition_point(tiles.begin(), tiles.end(), [&](const Tile &t) { return t.row0 < g.row_hi; });
  return TileRange{(uint32_t)(lo - tiles.begin()), (uint32_t)(hi - tiles.begin())};
}

// The output batches of a round, each with its tiles: what the fill launches of a round walk, for the host executor of the CPU tests
struct Group : pc::Group { uint32_t t_lo, t_hi; };
inline void plan_groups(const uint32_t *row_total, uint32_t nrows, uint64_t cap, const std::vector<Tile> &tiles, std::vector<Group> &out) {
  std::vector<pc::Group> rows;
  pc::plan_groups(row_total, 0, nrows, cap, rows);
  for (const pc::Group &g : rows) {
    const TileRange t = tile_range(g, tiles);
    Group G; static_cast<pc::Group &>(G) = g; G.t_lo = t.t_lo; G.t_hi = t.t_hi;
    out.push_back(G);
  }
}

}  // namespace ms
}  // namespace ckm
