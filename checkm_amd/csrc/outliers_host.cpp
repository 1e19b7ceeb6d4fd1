// outliers_host.cpp -- the tetranucleotide profile file of `checkm tetra` read once for `checkm outliers` (ABI 9): replaces
// GenomicSignatures.read (checkm/genomicSignatures.py:192-200), which BinTools.identifyOutliers calls once per bin
// (checkm/binTools.py:236-237).  Host code only: the lines are split over host threads at line ends.
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>
#include "ckm_internal.h"
#include "nucstats_host.h"
#include "outlier_dev.h"

using namespace ckm;

struct ckm_tetra_profile {
  std::vector<std::string> ids;
  std::vector<const char *> id_ptr;
  std::vector<double> val;                                   // [n * 136]
  std::unordered_map<std::string_view, uint32_t> index;      // keys point into ids
};

namespace {

constexpr int NSIG = ol::NSIG;

struct Chunk {
  std::vector<std::string> ids;
  std::vector<double> val;
  int err_code = 0;
  std::string err;
};

// float(token) for what the writer produces (the repr of a float64, 'nan', 'inf') with Python's tolerance of blanks around it: strtod is
// correctly rounded, as float() is.  Hexadecimal floats, which strtod would take and float() refuses, are refused.
bool parse_float(const char *a, const char *z, double &v) {
  while (a < z && (*a == ' ' || (*a >= '\t' && *a <= '\r'))) ++a;
  while (z > a && (z[-1] == ' ' || (z[-1] >= '\t' && z[-1] <= '\r'))) --z;
  if (a == z || z - a > 400) return false;
  char tmp[401];
  memcpy(tmp, a, (size_t)(z - a)); tmp[z - a] = 0;
  for (const char *p = tmp; *p; ++p) if (*p == 'x' || *p == 'X' || *p == '(') return false;
  char *end = nullptr;
  v = strtod(tmp, &end);
  return end == tmp + (z - a);
}

// lines of buf[a, z): a begins a line, z ends one (or the buffer)
void parse_lines(const std::string &buf, size_t a, size_t z, const char *path, Chunk &o) {
  const char *p = buf.data();
  size_t i = a;
  while (i < z) {
    size_t e = i; while (e < z && p[e] != '\n') ++e;
    const size_t next = e < z ? e + 1 : z;
    // line.split('\t'): the id is everything in front of the first tab (the line end stays on the last field and float() strips it)
    size_t t = i; while (t < e && p[t] != '\t') ++t;
    o.ids.emplace_back(p + i, (t < e ? t : e) - i);
    if (t >= e && !o.ids.back().empty() && o.ids.back().back() == '\r') o.ids.back().pop_back();
    int ncol = 0;
    size_t f = t < e ? t + 1 : e;
    const bool has_fields = t < e;
    while (has_fields) {
      size_t g = f; while (g < e && p[g] != '\t') ++g;
      double v;
      if (!parse_float(p + f, p + g, v)) {
        o.err_code = CKM_EFORMAT; o.err = std::string("not a float in column ") + std::to_string(ncol + 2) + " of sequence " + o.ids.back() + " in " + path; return;
      }
      if (ncol < NSIG) o.val.push_back(v);
      ++ncol;
      if (g >= e) break;
      f = g + 1;
    }
    if (ncol != NSIG) {
      o.err_code = CKM_EFORMAT;
      o.err = std::string("sequence ") + o.ids.back() + " has " + std::to_string(ncol) + " frequencies, not " + std::to_string(NSIG) + ", in " + path; return;
    }
    i = next;
  }
}

}  // namespace

extern "C" int ckm_tetra_profile_read(const char *path, ckm_tetra_profile **out) {
  try {
    if (!path || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::string buf, err;
    if (!read_bytes(path, buf, err)) throw Error(CKM_EIO, std::string("cannot read the tetranucleotide profile ") + path);
    size_t body = 0;                                         // next(f): the header line
    while (body < buf.size() && buf[body] != '\n') ++body;
    if (body < buf.size()) ++body;
    const size_t n = buf.size();
    const uint32_t nchunk = (uint32_t)std::min<size_t>(64, std::max<size_t>(1, (n - body) >> 20));
    std::vector<size_t> cut(nchunk + 1, n);
    cut[0] = body;
    for (uint32_t k = 1; k < nchunk; ++k) {
      size_t c = std::max(cut[k - 1], body + (n - body) / nchunk * k);
      while (c < n && buf[c] != '\n') ++c;
      cut[k] = c < n ? c + 1 : n;
    }
    std::vector<Chunk> chunks(nchunk);
    for_each_parallel(nchunk, [&](uint32_t k) {
      try { parse_lines(buf, cut[k], cut[k + 1], path, chunks[k]); }
      catch (const std::exception &e) { chunks[k].err_code = CKM_ENOMEM; chunks[k].err = e.what(); }
    });
    std::unique_ptr<ckm_tetra_profile> P(new ckm_tetra_profile);
    size_t total = 0;
    for (auto &c : chunks) { if (c.err_code) throw Error(c.err_code, c.err); total += c.ids.size(); }
    if (total > 0xFFFFFFF0ull) throw Error(CKM_ERANGE, "too many rows in the tetranucleotide profile");
    P->ids.reserve(total); P->val.reserve(total * NSIG); P->index.reserve(total);
    for (auto &c : chunks) {
      for (size_t r = 0; r < c.ids.size(); ++r) {
        auto it = P->index.find(std::string_view(c.ids[r]));
        if (it != P->index.end()) {                          // the dict keeps the id's place and takes the later row
          memcpy(&P->val[(size_t)it->second * NSIG], &c.val[r * NSIG], NSIG * sizeof(double));
          continue;
        }
        P->ids.push_back(std::move(c.ids[r]));               // (reserved: the strings never move again)
        P->index.emplace(std::string_view(P->ids.back()), (uint32_t)(P->ids.size() - 1));
        P->val.insert(P->val.end(), c.val.begin() + r * NSIG, c.val.begin() + (r + 1) * NSIG);
      }
      std::vector<std::string>().swap(c.ids); std::vector<double>().swap(c.val);
    }
    for (auto &s : P->ids) P->id_ptr.push_back(s.c_str());
    *out = P.release();
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

extern "C" int ckm_tetra_profile_view_get(const ckm_tetra_profile *p, ckm_tetra_profile_view *o) {
  if (!p || !o) { set_last_error("NULL argument"); return CKM_EINVAL; }
  o->n = (uint32_t)p->ids.size(); o->ids = p->id_ptr.data(); o->sig = p->val.data();
  return CKM_OK;
}

extern "C" int ckm_tetra_profile_gather(const ckm_tetra_profile *p, const ckm_nucseq *b, double *sig, int64_t *first_missing) {
  if (!p || !b || !sig || !first_missing) { set_last_error("NULL argument"); return CKM_EINVAL; }
  const uint32_t nseq = (uint32_t)b->ids.size();
  const uint32_t nblock = (nseq + 4095) / 4096;
  std::vector<int64_t> miss(std::max(1u, nblock), -1);
  for_each_parallel(nblock, [&](uint32_t k) {
    const uint32_t z = std::min(nseq, (k + 1) * 4096u);
    for (uint32_t s = k * 4096u; s < z; ++s) {
      auto it = p->index.find(std::string_view(b->ids[s]));
      if (it == p->index.end()) {
        if (miss[k] < 0) miss[k] = s;
        for (int c = 0; c < NSIG; ++c) sig[(size_t)s * NSIG + c] = 0.0;
      } else memcpy(sig + (size_t)s * NSIG, &p->val[(size_t)it->second * NSIG], NSIG * sizeof(double));
    }
  });
  *first_missing = -1;
  for (uint32_t k = 0; k < nblock; ++k) if (miss[k] >= 0) { *first_missing = miss[k]; break; }
  return CKM_OK;
}

extern "C" void ckm_tetra_profile_free(ckm_tetra_profile *p) { delete p; }
