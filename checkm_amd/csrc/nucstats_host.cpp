// nucstats_host.cpp -- host side of the nucleotide statistics (ABI 8): the FASTA reader with the rules of CheckM's readFasta
// (checkm/util/seqUtils.py:180-211) and the per-bin gene files BinStatistics.calculateCodingDensity reads (checkm/binStatistics.py:236-253).
// Host code only, a file per thread.
#include <sys/stat.h>
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "ckm_internal.h"
#include "nucstats_host.h"
#include "seqwin_dev.h"
#include "refdist_dev.h"

namespace ckm {

bool read_bytes(const char *path, std::string &buf, std::string &err) {
  const size_t n = strlen(path);
  if (n > 3 && !strcmp(path + n - 3, ".gz")) {                 // readFasta opens '.gz' names with gzip.open
    gzFile g = gzopen(path, "rb");
    if (!g) { err = std::string("cannot open FASTA file ") + path; return false; }
    char tmp[1 << 16];
    int got;
    while ((got = gzread(g, tmp, sizeof tmp)) > 0) buf.append(tmp, (size_t)got);
    int zerr = 0;
    const char *msg = gzerror(g, &zerr);
    gzclose(g);
    if (got < 0 || zerr < 0) { err = std::string("cannot decompress ") + path + ": " + (msg ? msg : "?"); return false; }
    return true;
  }
  FILE *f = fopen(path, "rb");
  if (!f) { err = std::string("cannot open FASTA file ") + path; return false; }
  fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
  buf.resize((size_t)std::max<long>(sz, 0));
  const size_t got = sz > 0 ? fread(&buf[0], 1, (size_t)sz, f) : 0;
  fclose(f);
  if ((long)got != sz) { err = std::string("short read on ") + path; return false; }
  return true;
}

// Python's utf-8 decoder: no overlong forms, no surrogates, nothing above U+10FFFF.  Returns the offset of the first bad byte or npos.
static size_t utf8_invalid_at(const std::string &s) {
  const unsigned char *p = (const unsigned char *)s.data();
  const size_t n = s.size();
  size_t i = 0;
  while (i < n) {
    const unsigned c = p[i];
    if (c < 0x80) { ++i; continue; }
    int len; unsigned lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) len = 2;
    else if (c >= 0xE0 && c <= 0xEF) { len = 3; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { len = 4; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    else return i;
    if (i + len > n) return i;
    if (p[i + 1] < lo || p[i + 1] > hi) return i;
    for (int k = 2; k < len; ++k) if (p[i + k] < 0x80 || p[i + k] > 0xBF) return i;
    i += len;
  }
  return std::string::npos;
}

// str.isspace() of the code point starting at p (UTF-8, already validated); *len = its bytes
static bool py_space(const unsigned char *p, int *len) {
  const unsigned c = p[0];
  if (c < 0x80) { *len = 1; return c == ' ' || (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x1F); }
  uint32_t cp; int n;
  if (c < 0xE0) { cp = c & 0x1F; n = 2; } else if (c < 0xF0) { cp = c & 0x0F; n = 3; } else { cp = c & 0x07; n = 4; }
  for (int k = 1; k < n; ++k) cp = (cp << 6) | (p[k] & 0x3F);
  *len = n;
  return cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) || cp == 0x2028 || cp == 0x2029 || cp == 0x202F ||
         cp == 0x205F || cp == 0x3000;
}

// line i..e (without its terminator) of a file opened in text mode.  keep_text = false (ckm_fasta_ids_read): the same rules, but of a
// sequence only its bytes and code points are kept (o.nbytes, o.ncp), never its text.
static void parse_nuc_fasta(const char *path, NucFile &o, bool keep_text = true) {
  std::string buf;
  if (!read_bytes(path, buf, o.err)) { o.err_code = CKM_EIO; return; }
  const size_t bad = utf8_invalid_at(buf);
  if (bad != std::string::npos) {
    o.err_code = CKM_EFORMAT; o.err = std::string("invalid UTF-8 at byte ") + std::to_string(bad) + " of " + path; return;
  }
  std::unordered_map<std::string, uint32_t> index;
  const unsigned char *p = (const unsigned char *)buf.data();
  const size_t n = buf.size();
  long cur = -1;
  size_t i = 0;
  while (i < n) {
    size_t e = i; while (e < n && p[e] != '\n' && p[e] != '\r') ++e;
    const bool term = e < n;                                   // universal newlines: "\n", "\r\n" and a lone "\r" end a line
    const size_t next = !term ? n : (p[e] == '\r' && e + 1 < n && p[e + 1] == '\n') ? e + 2 : e + 1;
    bool blank = true;                                         // `if not line.strip(): continue`
    for (size_t k = i; k < e && blank;) { int l; if (!py_space(p + k, &l)) blank = false; k += l; }
    if (!blank) {
      if (p[i] == '>') {                                       // seqId = line[1:].split(None, 1)[0]
        size_t a = i + 1; int l = 1;
        while (a < e && py_space(p + a, &l)) a += l;
        size_t z = a;
        while (z < e && !py_space(p + z, &l)) z += l;
        if (z == a) { o.err_code = CKM_EFORMAT; o.err = std::string("header without an id in ") + path; return; }
        std::string id((const char *)p + a, z - a);
        auto it = index.find(id);
        if (it == index.end()) {                               // a repeated id keeps its place and takes the later record
          index.emplace(id, (uint32_t)o.ids.size()); cur = (long)o.ids.size(); o.ids.push_back(std::move(id));
          if (keep_text) o.seqs.emplace_back(); else { o.nbytes.push_back(0); o.ncp.push_back(0); }
        } else if (keep_text) { cur = (long)it->second; o.seqs[cur].clear(); }
        else { cur = (long)it->second; o.nbytes[cur] = 0; o.ncp[cur] = 0; }
      } else {
        if (cur < 0) { o.err_code = CKM_EFORMAT; o.err = std::string("sequence text before the first header in ") + path; return; }
        size_t z = e;                                          // line[0:-1]: the terminator, or the last character of the file
        if (!term) { do { --z; } while (z > i && (p[z] & 0xC0) == 0x80); }
        if (keep_text) o.seqs[cur].append((const char *)p + i, z - i);
        else { o.nbytes[cur] += z - i; o.ncp[cur] += sw::code_points((const char *)p, i, z - i); }
      }
    }
    i = next;
  }
}


// ---- the genes of one bin ----------------------------------------------------------------------------------------------------------------
// ProdigalGeneFeatureParser (checkm_amd/prodigal.py, the restatement of checkm/prodigal.py:208-274): per sequence id the genes keyed by
// <id>_<counter> (the counter restarts whenever a NEW id appears, so a later gene can replace an earlier one of the same key), the last
// coding base, and the union of the intervals up to it.
struct GffSeq { std::unordered_map<long, std::pair<long long, long long>> genes; long long last = 0; };

// The rows of one GFF file.  A file that does not exist: *missing = true and nothing else.
static int parse_gff(const char *gff, std::unordered_map<std::string, GffSeq> &seqs, bool &have_table, long &tt, bool &missing, std::string &err) {
  struct stat sb;
  missing = stat(gff, &sb) != 0;
  if (missing) return CKM_OK;
  std::string buf;
  if (!read_bytes(gff, buf, err)) return CKM_EIO;
  long counter = 0;
  have_table = false; tt = 0;
  size_t i = 0; const size_t n = buf.size();
  while (i < n) {
    size_t e = i; while (e < n && buf[e] != '\n' && buf[e] != '\r') ++e;
    const size_t next = e >= n ? n : (buf[e] == '\r' && e + 1 < n && buf[e + 1] == '\n') ? e + 2 : e + 1;
    const std::string line = buf.substr(i, e - i);
    i = next;
    if (line.compare(0, 12, "# Model Data") == 0 && (!have_table || tt == 0)) {
      size_t a = 0;
      while (a <= line.size()) {
        size_t z = line.find(';', a); if (z == std::string::npos) z = line.size();
        const std::string tok = line.substr(a, z - a);
        if (tok.find("transl_table") != std::string::npos) {
          const size_t eq = tok.find('=');
          tt = strtol(tok.c_str() + (eq == std::string::npos ? 0 : eq + 1), nullptr, 10); have_table = true;
        }
        a = z + 1;
      }
    }
    if (line.empty() || line[0] == '#') continue;
    { size_t a = line.find_first_not_of(" \t\v\f"), z = line.find_last_not_of(" \t\v\f"); if (a != std::string::npos && z == a && line[a] == '"') continue; }
    size_t c[5]; size_t pos = 0; int nc = 0;
    for (; nc < 5; ++nc) { c[nc] = pos; const size_t t = line.find('\t', pos); if (t == std::string::npos) { ++nc; break; } pos = t + 1; }
    if (nc < 5) { err = std::string("GFF line with fewer than five columns in ") + gff; return CKM_EFORMAT; }
    const std::string id = line.substr(0, line.find('\t'));
    auto it = seqs.find(id);
    if (it == seqs.end()) { counter = 0; it = seqs.emplace(id, GffSeq()).first; }
    const long long s = strtoll(line.c_str() + c[3], nullptr, 10), z = strtoll(line.c_str() + c[4], nullptr, 10);
    it->second.genes[counter++] = {s, z};
    it->second.last = std::max(it->second.last, z);
  }
  return CKM_OK;
}

// The coding-base mask of one sequence (ProdigalGeneFeatureParser._buildCodingBaseMask) as disjoint ascending intervals [lo, hi): the
// union of its genes, clipped to [0, last coding base)
static void merged_intervals(const GffSeq &g, std::vector<std::pair<long long, long long>> &out) {
  std::vector<std::pair<long long, long long>> iv;
  for (auto &x : g.genes) if (x.second.second > x.second.first - 1) iv.push_back({x.second.first - 1, x.second.second});
  std::sort(iv.begin(), iv.end());
  const long long last = g.last;
  long long cs = 0, ce = -1; bool open = false;
  auto flush = [&] { if (open) { const long long lo = std::max(cs, 0LL), hi = std::min(ce, last); if (hi > lo) out.push_back({lo, hi}); } };
  for (auto &v : iv) {
    if (open && v.first <= ce) ce = std::max(ce, v.second);
    else { flush(); cs = v.first; ce = v.second; open = true; }
  }
  flush();
}

// ProdigalGeneFeatureParser.codingBases(seqId): bases of one sequence inside the union of its genes
static long long coding_bases(const GffSeq &g) {
  std::vector<std::pair<long long, long long>> iv;
  merged_intervals(g, iv);
  long long total = 0;
  for (auto &v : iv) total += v.second - v.first;
  return total;
}

static int read_bin_genes(const char *gff, const char *faa, const std::vector<std::string> &ids, int64_t &coding, int32_t &table, int64_t &ngenes, std::string &err) {
  std::unordered_map<std::string, GffSeq> seqs;
  bool have_table = false, missing = false; long tt = 0;
  const int prc = parse_gff(gff, seqs, have_table, tt, missing, err);
  if (prc) return prc;
  if (missing) { coding = -1; table = -1; ngenes = -1; return CKM_OK; }
  size_t i = 0;
  // bases of the bin's sequences inside the union of their genes
  std::unordered_set<std::string> seen;
  long long total = 0;
  for (const std::string &id : ids) {
    if (!seen.insert(id).second) continue;
    auto it = seqs.find(id);
    if (it != seqs.end()) total += coding_bases(it->second);
  }
  // len(readFasta(genes.faa)): distinct ids
  std::string fbuf;
  if (!read_bytes(faa, fbuf, err)) return CKM_EIO;
  std::unordered_set<std::string> names;
  i = 0;
  const size_t fn = fbuf.size();
  while (i < fn) {
    size_t e = i; while (e < fn && fbuf[e] != '\n' && fbuf[e] != '\r') ++e;
    if (e > i && fbuf[i] == '>') {
      size_t a = i + 1; while (a < e && isspace((unsigned char)fbuf[a])) ++a;
      size_t z = a; while (z < e && !isspace((unsigned char)fbuf[z])) ++z;
      names.emplace(fbuf.data() + a, z - a);
    }
    i = e >= fn ? fn : (fbuf[e] == '\r' && e + 1 < fn && fbuf[e + 1] == '\n') ? e + 2 : e + 1;
  }
  coding = total; table = have_table ? (int32_t)tt : INT32_MIN; ngenes = (int64_t)names.size();
  return CKM_OK;
}

}  // namespace ckm
using namespace ckm;

extern "C" int ckm_nucseq_read(const char *const *paths, uint32_t nfiles, ckm_nucseq **out) {
  try {
    if (!out || (nfiles && !paths)) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::vector<NucFile> files(nfiles);
    for_each_parallel(nfiles, [&](uint32_t b) {
      if (!paths[b]) { files[b].err_code = CKM_EINVAL; files[b].err = "NULL path"; return; }
      parse_nuc_fasta(paths[b], files[b]);
    });
    std::unique_ptr<ckm_nucseq> B(new ckm_nucseq);
    uint64_t pos = 0;
    B->file_first.push_back(0);
    for (auto &f : files) {
      if (f.err_code) throw Error(f.err_code, f.err);
      for (size_t s = 0; s < f.seqs.size(); ++s) {
        B->seq_off.push_back(pos); B->seq_bytes.push_back(f.seqs[s].size());
        pos += (f.seqs[s].size() + 15) & ~(uint64_t)15;
      }
      B->file_first.push_back((uint32_t)B->seq_off.size());
    }
    B->text.assign(pos + 64, 0);                               // 16-byte aligned sequences, zero padding, 64 bytes of slack
    size_t k = 0;
    for (auto &f : files) {
      for (size_t s = 0; s < f.seqs.size(); ++s, ++k) {
        if (!f.seqs[s].empty()) memcpy(&B->text[B->seq_off[k]], f.seqs[s].data(), f.seqs[s].size());
        std::string().swap(f.seqs[s]);
        B->ids.push_back(std::move(f.ids[s]));
      }
    }
    for (auto &s : B->ids) B->id_ptr.push_back(s.c_str());
    B->seq_cp.assign(B->seq_off.size(), 0);
    for_each_parallel((uint32_t)B->seq_off.size(), [&](uint32_t s) { B->seq_cp[s] = sw::code_points(B->text.data(), B->seq_off[s], B->seq_bytes[s]); });
    *out = B.release();
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

// The ids and lengths of FASTA files by the rules of ckm_nucseq_read, without their text: a file per thread, each file's buffer freed
// when its thread is done with it.
extern "C" int ckm_fasta_ids_read(const char *const *paths, uint32_t nfiles, ckm_fasta_ids **out) {
  try {
    if (!out || (nfiles && !paths)) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::vector<NucFile> files(nfiles);
    for_each_parallel(nfiles, [&](uint32_t b) {
      if (!paths[b]) { files[b].err_code = CKM_EINVAL; files[b].err = "NULL path"; return; }
      try { parse_nuc_fasta(paths[b], files[b], false); }
      catch (const std::exception &e) { files[b].err_code = CKM_ENOMEM; files[b].err = e.what(); }
    });
    std::unique_ptr<ckm_fasta_ids> B(new ckm_fasta_ids);
    B->file_first.push_back(0);
    for (auto &f : files) {
      if (f.err_code) throw Error(f.err_code, f.err);
      for (size_t s = 0; s < f.ids.size(); ++s) {
        B->ids.push_back(std::move(f.ids[s])); B->seq_bytes.push_back(f.nbytes[s]); B->seq_cp.push_back(f.ncp[s]);
      }
      B->file_first.push_back((uint32_t)B->ids.size());
    }
    for (auto &s : B->ids) B->id_ptr.push_back(s.c_str());
    *out = B.release();
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

extern "C" int ckm_fasta_ids_view_get(const ckm_fasta_ids *b, ckm_fasta_ids_view *o) {
  if (!b || !o) { set_last_error("NULL argument"); return CKM_EINVAL; }
  o->seq_ids = b->id_ptr.data(); o->seq_bytes = b->seq_bytes.data(); o->seq_cp = b->seq_cp.data(); o->file_first = b->file_first.data();
  o->nseq = (uint32_t)b->ids.size(); o->nfiles = (uint32_t)b->file_first.size() - 1;
  return CKM_OK;
}

extern "C" void ckm_fasta_ids_free(ckm_fasta_ids *b) { delete b; }

extern "C" int ckm_nucseq_view_get(const ckm_nucseq *b, ckm_nucseq_view *o) {
  if (!b || !o) { set_last_error("NULL argument"); return CKM_EINVAL; }
  o->text = b->text.data(); o->text_bytes = b->text.size();
  o->seq_off = b->seq_off.data(); o->seq_bytes = b->seq_bytes.data(); o->file_first = b->file_first.data(); o->seq_ids = b->id_ptr.data();
  o->nseq = (uint32_t)b->seq_off.size(); o->nfiles = (uint32_t)b->file_first.size() - 1;
  return CKM_OK;
}

extern "C" void ckm_nucseq_free(ckm_nucseq *b) { delete b; }

// Per sequence what ckm_bin_genes_read sums per file: ProdigalGeneFeatureParser.codingBases(seqId), 0 for an id without genes.
extern "C" int ckm_seq_genes_read(const char *const *gff_paths, const ckm_nucseq *b, int64_t *coding_per_seq, uint8_t *missing) {
  if (!gff_paths || !b || !coding_per_seq || !missing) { set_last_error("NULL argument"); return CKM_EINVAL; }
  const uint32_t nb = (uint32_t)b->file_first.size() - 1;
  std::vector<int> rc(nb, CKM_OK);
  std::vector<std::string> err(nb);
  for_each_parallel(nb, [&](uint32_t k) {
    try {
      if (!gff_paths[k]) { rc[k] = CKM_EINVAL; err[k] = "NULL path"; return; }
      std::unordered_map<std::string, GffSeq> seqs;
      bool have_table = false, miss = false; long tt = 0;
      rc[k] = parse_gff(gff_paths[k], seqs, have_table, tt, miss, err[k]);
      missing[k] = miss ? 1 : 0;
      if (rc[k]) return;
      for (uint32_t s = b->file_first[k]; s < b->file_first[k + 1]; ++s) {
        if (miss) { coding_per_seq[s] = -1; continue; }
        auto it = seqs.find(b->ids[s]);
        coding_per_seq[s] = it == seqs.end() ? 0 : (int64_t)coding_bases(it->second);
      }
    } catch (const std::exception &e) { rc[k] = CKM_ENOMEM; err[k] = e.what(); }
  });
  for (uint32_t k = 0; k < nb; ++k)
    if (rc[k]) { set_last_error(err[k]); return rc[k]; }
  return CKM_OK;
}

extern "C" int ckm_bin_genes_read(const char *const *gff_paths, const char *const *faa_paths, const ckm_nucseq *b,
                                  int64_t *coding, int32_t *trans_table, int64_t *ngenes) {
  if (!gff_paths || !faa_paths || !b || !coding || !trans_table || !ngenes) { set_last_error("NULL argument"); return CKM_EINVAL; }
  const uint32_t nb = (uint32_t)b->file_first.size() - 1;
  std::vector<int> rc(nb, CKM_OK);
  std::vector<std::string> err(nb);
  for_each_parallel(nb, [&](uint32_t k) {
    std::vector<std::string> ids(b->ids.begin() + b->file_first[k], b->ids.begin() + b->file_first[k + 1]);
    try { rc[k] = read_bin_genes(gff_paths[k], faa_paths[k], ids, coding[k], trans_table[k], ngenes[k], err[k]); }
    catch (const std::exception &e) { rc[k] = CKM_ENOMEM; err[k] = e.what(); }
  });
  for (uint32_t k = 0; k < nb; ++k)
    if (rc[k]) { set_last_error(err[k]); return rc[k]; }
  return CKM_OK;
}

// ---- the windows of the plot commands (seqwin_dev.h) ----------------------------------------------------------------------------------
namespace ckm {
void window_layout(const ckm_nucseq *b, uint64_t w, std::vector<uint64_t> &first) {
  if (!sw::window_layout(b->seq_cp.data(), (uint32_t)b->seq_cp.size(), w, first))
    throw Error(CKM_ERANGE, "more than 2^31 - 1 windows in one call: use a larger window or fewer files");
}
}  // namespace ckm

extern "C" int ckm_seq_windows_layout(const ckm_nucseq *b, int64_t window_size, int64_t *out_first) {
  try {
    if (!b || !out_first) throw Error(CKM_EINVAL, "NULL argument");
    if (window_size < 1 || (uint64_t)window_size > sw::MAX_WINDOWS) throw Error(CKM_EINVAL, "window_size must be between 1 and 2^31 - 1");
    std::vector<uint64_t> first;
    window_layout(b, (uint64_t)window_size, first);
    for (size_t k = 0; k < first.size(); ++k) out_first[k] = (int64_t)first[k];
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

// np.sum(mask[k w : (k + 1) w]) for every window of every sequence: the merged intervals against the window bounds, O(intervals + windows)
extern "C" int ckm_seq_windows_coding(const char *const *gff_paths, const ckm_nucseq *b, int64_t window_size, int64_t *out_coding, uint8_t *missing) {
  try {
    if (!gff_paths || !b || !out_coding || !missing) throw Error(CKM_EINVAL, "NULL argument");
    if (window_size < 1 || (uint64_t)window_size > sw::MAX_WINDOWS) throw Error(CKM_EINVAL, "window_size must be between 1 and 2^31 - 1");
    const long long w = (long long)window_size;
    std::vector<uint64_t> first;
    window_layout(b, (uint64_t)w, first);
    const uint32_t nb = (uint32_t)b->file_first.size() - 1;
    std::vector<int> rc(nb, CKM_OK);
    std::vector<std::string> err(nb);
    for_each_parallel(nb, [&](uint32_t k) {
      try {
        if (!gff_paths[k]) { rc[k] = CKM_EINVAL; err[k] = "NULL path"; return; }
        std::unordered_map<std::string, GffSeq> seqs;
        bool have_table = false, miss = false; long tt = 0;
        rc[k] = parse_gff(gff_paths[k], seqs, have_table, tt, miss, err[k]);
        missing[k] = miss ? 1 : 0;
        if (rc[k]) return;
        std::vector<std::pair<long long, long long>> iv;
        for (uint32_t s = b->file_first[k]; s < b->file_first[k + 1]; ++s) {
          const long long nw = (long long)(first[s + 1] - first[s]);
          int64_t *out = out_coding + first[s];
          for (long long x = 0; x < nw; ++x) out[x] = miss ? -1 : 0;
          if (miss || !nw) continue;
          auto it = seqs.find(b->ids[s]);
          if (it == seqs.end()) continue;
          iv.clear();
          merged_intervals(it->second, iv);
          for (auto &v : iv) {
            if (v.first / w >= nw) break;                      // ascending: nothing behind it reaches a window either
            const long long z = std::min((v.second - 1) / w, nw - 1);
            for (long long x = v.first / w; x <= z; ++x)
              out[x] += std::min(v.second, (x + 1) * w) - std::max(v.first, x * w);
          }
        }
      } catch (const std::bad_alloc &) { rc[k] = CKM_ENOMEM; err[k] = "out of host memory"; }
      catch (const std::exception &e) { rc[k] = CKM_EINVAL; err[k] = e.what(); }
    });
    for (uint32_t k = 0; k < nb; ++k)
      if (rc[k]) { set_last_error(err[k]); return rc[k]; }
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

// ---- the windows of the reference distributions (refdist_dev.h) --------------------------------------------------------------------------
extern "C" int ckm_refdist_check(int stat, uint32_t sep_len, uint32_t block, uint64_t scaffold_len, const int64_t *starts, const int64_t *sizes, uint64_t nwin) {
  try {
    const std::string refusal = rd::check_args(stat, sep_len, block, scaffold_len, starts, sizes, nwin);
    if (!refusal.empty()) throw Error(rd::refusal_code(scaffold_len, nwin), refusal);
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}

// np.sum(mask[start : start + size]) for windows anywhere in one sequence: the merged intervals and the coding bases in front of each,
// a binary search per window end
extern "C" int ckm_refdist_coding(const char *gff_path, const char *seq_id, const int64_t *starts, const int64_t *sizes, uint64_t nwin, int64_t *out_coding,
                                  int64_t *out_total) {
  try {
    if (!gff_path || !seq_id || !out_total || (nwin && (!starts || !sizes || !out_coding))) throw Error(CKM_EINVAL, "NULL argument");
    std::unordered_map<std::string, GffSeq> seqs;
    bool have_table = false, miss = false; long tt = 0;
    std::string err;
    const int rc = parse_gff(gff_path, seqs, have_table, tt, miss, err);
    if (rc) throw Error(rc, err);
    if (miss) throw Error(CKM_EIO, std::string("cannot read ") + gff_path);
    std::vector<std::pair<long long, long long>> iv;
    auto it = seqs.find(seq_id);
    if (it != seqs.end()) merged_intervals(it->second, iv);
    std::vector<long long> before(iv.size() + 1, 0);          // coding bases in front of interval k
    for (size_t k = 0; k < iv.size(); ++k) before[k + 1] = before[k] + (iv[k].second - iv[k].first);
    // coding bases in [0, p)
    auto upto = [&](long long p) {
      const size_t k = (size_t)(std::upper_bound(iv.begin(), iv.end(), std::make_pair(p, (long long)0x7FFFFFFFFFFFFFFFLL)) - iv.begin());   // intervals with first <= p
      if (k == 0) return 0LL;
      return before[k - 1] + (std::min(p, iv[k - 1].second) - iv[k - 1].first);
    };
    for (uint64_t x = 0; x < nwin; ++x) {
      if (starts[x] < 0 || sizes[x] < 0 || sizes[x] > 0x7FFFFFFFFFFFFFFFLL - starts[x]) throw Error(CKM_EINVAL, "window " + std::to_string(x) + " is no range of a sequence");
      out_coding[x] = (int64_t)(upto(starts[x] + sizes[x]) - upto(starts[x]));
    }
    *out_total = (int64_t)before[iv.size()];
    return CKM_OK;
  } catch (const Error &e) { set_last_error(e.what()); return e.code; }
  catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
  catch (const std::exception &e) { set_last_error(e.what()); return CKM_EINVAL; }
}
