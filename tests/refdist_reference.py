"""TEST INFRASTRUCTURE: a plain-Python restatement of the intended semantics of CheckM's table-building scripts
(scripts/distributionDeltaGC.py, distributionDeltaCodingDensity.py, distributionDeltaTetraDiff.py, calculateBounds.py,
calculateBoundsTD.py) as DESIGN §18 states them: slices and str.count, a dict of 4-mers, a numpy mask, np.percentile.
tests/test_refdist_host.py pins it to what the reference's own seqSignature / distance / codingBases / readFasta give when driven
through the same loops (tests/golden/refdist_cases.json)."""
import os
import random

import numpy as np

from tests.seqwin_reference import KMER_INDEX, coding_masks, signature

SEPARATOR = {"gc": "", "td": "NNNN", "cd": "N" * 10}
DRAW_LIMIT = 100                                            # draws of one size per wanted window before the size is given up


def window_sizes():
    sizes = []
    for a, z, step in ((500, 1000, 100), (1000, 2000, 200), (2000, 5000, 500), (5000, 10000, 1000), (10000, 50000, 5000), (50000, 100000, 10000),
                       (100000, 400000, 100000), (400000, 1000001, 200000)):
        sizes += list(range(a, z, step))
    return sizes


def genome_id(path):
    name = os.path.basename(path)
    return name[0:name.rfind(".")] if "." in name else name


def scaffold(seqs, stat):
    s = SEPARATOR[stat].join(seqs.values())
    return s if stat == "td" else s.upper()                 # seqSignature upper-cases on its own


def scaffold_file(seqs, genomeId):
    return ">" + genomeId + "\n" + scaffold(seqs, "cd")


def stream(seed, genomeId, stat, w):
    return random.Random("%s:%s:%s:%d" % (seed, genomeId, stat, w))


def no_window_error(genomeId, stat, w, numWindows):
    return ValueError("genome %s: fewer than %d acceptable %s windows of size %d in %d draws" % (genomeId, numWindows, stat, w, DRAW_LIMIT * numWindows))


def sample(L, sizes, numWindows, seed, genomeId, stat, value):
    """{w: [values]}: the scripts' loop.  value(s, w) is the window's number, or None for a window the script skips."""
    out = {}
    for w in sizes:
        if L - w <= 0:
            break
        r, vals, draws = stream(seed, genomeId, stat, w), [], 0
        while len(vals) != numWindows:
            if draws == DRAW_LIMIT * numWindows:
                raise no_window_error(genomeId, stat, w, numWindows)
            s = r.randint(0, L - w)
            draws += 1
            v = value(s, w)
            if v is not None:
                vals.append(v)
        out[w] = vals
    return out


def gc_at(s):
    return s.count("C") + s.count("G"), s.count("A") + s.count("T") + s.count("U")


def delta_gc(seqs, genomeId, numWindows, sizes, seed):
    scaf = scaffold(seqs, "gc")
    gc, at = gc_at(scaf)
    meanGC = float(gc) / (gc + at)

    def value(s, w):
        g, a = gc_at(scaf[s:s + w])
        if g + a < 0.9 * w:
            return None
        return float(g) / (g + a) - meanGC
    return meanGC, sample(len(scaf), sizes, numWindows, seed, genomeId, "gc", value)


def delta_cd(seqs, gff_text, genomeId, numWindows, sizes, seed):
    scaf = scaffold(seqs, "cd")
    mask = coding_masks(gff_text).get(genomeId)
    gc, at = gc_at(scaf)
    meanCD = float(np.sum(mask) if mask is not None else 0) / (gc + at)

    def value(s, w):
        g, a = gc_at(scaf[s:s + w])
        if g + a != w:
            return None
        return float(np.sum(mask[s:s + w]) if mask is not None else 0) / (g + a) - meanCD
    return meanCD, sample(len(scaf), sizes, numWindows, seed, genomeId, "cd", value)


def delta_td(seqs, genomeId, numWindows, sizes, seed):
    scaf = scaffold(seqs, "td")
    genomeSig = signature(scaf)

    def value(s, w):
        return float(np.sum(np.abs(genomeSig - signature(scaf[s:s + w]))))
    return genomeSig, sample(len(scaf), sizes, numWindows, seed, genomeId, "td", value)


def delta_td_numpy(seqs, genomeId, numWindows, sizes, seed):
    """delta_td for genomes too long for a Python loop per base: the canonical column of the 4-mer starting at every position is
    looked up once, a window is a bincount over a slice of them.  test_refdist_host.py pins it to delta_td."""
    scaf = scaffold(seqs, "td")
    code = np.full(256, -1, dtype=np.int64)
    for k, c in enumerate("ACGT"):
        code[ord(c)] = code[ord(c.lower())] = k
    b = code[np.frombuffer(scaf.encode("latin-1", "replace"), dtype=np.uint8)]
    col = np.full(max(0, len(b) - 3), -1, dtype=np.int64)
    if len(col):
        table = np.array([KMER_INDEX[a + c + g + t] for a in "ACGT" for c in "ACGT" for g in "ACGT" for t in "ACGT"])
        ok = (b[:-3] >= 0) & (b[1:-2] >= 0) & (b[2:-1] >= 0) & (b[3:] >= 0)
        col[ok] = table[(b[:-3] * 64 + b[1:-2] * 16 + b[2:-1] * 4 + b[3:])[ok]]

    def sig_of(s, e):
        c = col[s:max(s, e - 3)]
        sig = np.bincount(c[c >= 0], minlength=136).astype(float)
        with np.errstate(invalid="ignore"):
            sig /= np.sum(sig)
        return sig
    genomeSig = sig_of(0, len(scaf))

    def value(s, w):
        return float(np.sum(np.abs(genomeSig - sig_of(s, s + w))))
    return genomeSig, sample(len(scaf), sizes, numWindows, seed, genomeId, "td", value)


def file_text(stat, head, dist):
    if stat == "td":
        text = "# Tetra signature = " + ",".join(str(float(v)) for v in head) + "\n"
    else:
        text = "# Mean %s = %s\n" % (stat.upper(), str(float(head)))
    for w, vals in dist.items():
        text += "Windows Size = " + str(w) + "\n" + ",".join(str(float(v)) for v in vals) + "\n"
    return text


def read_windows(text):
    """[(windowSize, line)] of one per-genome file."""
    out, w = [], None
    for line in text.splitlines():
        if "Windows Size" in line:
            w = int(line.split("=")[1].strip())
        elif w is not None:
            out.append((w, line))
            w = None
    return out


CIS = np.arange(0, 100 + 0.5, 0.5).tolist()


def percentiles(pts):
    return {ci: float(p) for ci, p in zip(CIS, np.percentile(np.array(pts), CIS))}


def bounds(files, stepSize=0.01, width=0.015, minGenomes=5):
    """files: {genomeId: text of its deltaGC or deltaCD file}.  {mean: {windowSize: {percentile: value}}}."""
    means = {g: float(files[g].split("\n", 1)[0].split("=")[1]) for g in sorted(files)}
    out = {}
    for centre in np.arange(0.0, 1.0 + 0.5 * stepSize, stepSize):
        ids = [g for g, v in means.items() if v >= centre - width and v <= centre + width]
        if len(ids) < minGenomes:
            continue
        d = {}
        for g in ids:
            for w, line in read_windows(files[g]):
                d.setdefault(w, []).extend(float(x) for x in line.split(","))
        out[float(centre)] = {w: percentiles(pts) for w, pts in d.items()}
    return out


def bounds_td(files, seed, cap=10000):
    """({windowSize: {percentile: value}}, bad genome ids)."""
    windows, bad = {}, []
    for g in sorted(files):
        for w, line in read_windows(files[g]):
            if "nan" in line:
                if g not in bad:
                    bad.append(g)
                continue
            vals = [float(x) for x in line.split(",")]
            if len(vals) > cap:
                vals = random.Random("%s:%s:%d" % (seed, g, w)).sample(vals, cap)
            windows.setdefault(w, []).extend(vals)
    return {w: percentiles(pts) for w, pts in windows.items()}, bad
