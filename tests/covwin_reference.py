"""TEST INFRASTRUCTURE: CoverageWindows restated in plain Python -- the BAM reader of tests/shim/pysam_legacy.py, the elif chain of
checkm/coverageWindows.py:55-79 and a per-base numpy depth array summed window by window, as the reference does.  A second formulation,
independent of the difference arrays of the library (checkm_amd/csrc/covwin_dev.h).  tests/test_covwin_host.py pins it to the goldens,
which the reference's own CoverageWindows wrote on the same shim (tools/gen_covwin_golden.py).  Also what the tests share: the
synthetic record generator of the structure tests and the loader of the goldens."""
import json
import os
import random

import numpy as np

from synthdata import bam as sbam
from tests.shim import pysam_legacy as shim

PARAMS = (False, 0.98, 0.02)          # bAllReads, minAlignPer, maxEditDistPer


def classify(read, bAllReads, minAlignPer, maxEditDistPer):
    """Class 0..7 of one read of the shim: the reference's chain, in its order."""
    if read.is_unmapped:
        return 0
    elif read.is_duplicate:
        return 1
    elif read.is_secondary:
        return 2
    elif read.is_qcfail:
        return 3
    elif read.alen < minAlignPer * read.rlen:
        return 4
    elif read.opt('NM') > maxEditDistPer * read.rlen:
        return 5
    elif not bAllReads and not read.is_proper_pair:
        return 6
    return 7


def depth(path, bAllReads, minAlignPer, maxEditDistPer, classes=None, mapped=None):
    """(references, lengths, [n_ref, 9] int64 counters, [per-base float64 depth per reference]).  `classes` (a list) receives the class
    of every record with a reference, `mapped` the (ref, pos, alen) of every mapped one."""
    f = shim.Samfile(path, 'rb')
    out = np.zeros((len(f.references), 9), dtype=np.int64)
    cov = [np.zeros(n) for n in f.lengths]
    for r in f._reads:
        if r.reference_id < 0:
            continue
        c = classify(r, bAllReads, minAlignPer, maxEditDistPer)
        if classes is not None:
            classes.append(c)
        out[r.reference_id, 0] += 1
        if c:
            out[r.reference_id, c] += 1
        if c == 7:
            assert r.pos >= 0
            cov[r.reference_id][r.pos:r.pos + r.alen] += 1.0
            if mapped is not None:
                mapped.append((r.reference_id, r.pos, r.alen))
    for k, d in enumerate(cov):
        out[k, 8] = int(d.sum())
    return list(f.references), list(f.lengths), out, cov


def slots(cov, w):
    """(first[n_ref + 1], the sum of the depth over every slot of every reference: its reported windows and the tail) as int64."""
    first, sums = [0], []
    for d in cov:
        n = (len(d) - 1) // w + 1 if len(d) else 0
        sums += [int(d[k * w:(k + 1) * w].sum()) for k in range(n)]
        first.append(len(sums))
    return np.array(first, dtype=np.int64), np.array(sums, dtype=np.int64)


def run(path, params, w):
    """({seqId: [coverage, windowCoverages]}, counters) as the reference's worker computes them (coverageWindows.py:185-200)."""
    refs, lens, cnt, cov = depth(path, *params)
    info = {}
    for seqId, seqLen, d in zip(refs, lens, cov):
        start, end, wc = 0, w, []
        while end < seqLen:
            wc.append(float(sum(d[start:end]) / w))
            start = end
            end += w
        info[seqId] = [float(sum(d)) / seqLen, wc]
    return info, cnt


def hexed(info):
    return {k: [v[0].hex(), [x.hex() for x in v[1]]] for k, v in info.items()}


def synthetic(nrec, nref, seed, w=100, interleave=False, run_lengths=None, ref_len=None):
    """(refs, records): the records of synthdata.bam.synthetic (an eighth of the reads in each class of the OTHER chain under its PARAMS)
    re-dressed for this chain and for the window geometry: sorted positions inside each reference, a fifth of the reads with a deletion
    or an N that spans windows, reads that run past the reference's end, supplementary reads that stay mapped, and QC by flag only."""
    refs, recs = sbam.synthetic(nrec, nref, seed, run_lengths=run_lengths)
    r = random.Random(seed * 7919 + 1)
    if ref_len is not None:
        refs = [(n, ref_len(k)) for k, (n, _l) in enumerate(refs)]
    by = {}
    for x in recs:
        by.setdefault(x["ref"], []).append(x)
    for ref, lst in by.items():
        L = refs[ref][1]
        pos = sorted(r.randrange(max(1, L)) for _ in lst)
        for x, p in zip(lst, pos):
            x["pos"] = p if r.random() >= 0.03 else L + r.randrange(3)            # starts at or past the end: covers nothing
            m = x["l_seq"] - sum(n for op, n in x["cigar"] if op == "S")
            u = r.random()
            mid = [("M", m)]
            if u < 0.10:
                mid = [("M", m // 2), ("D", r.randrange(1, w)), ("M", m - m // 2)]
            elif u < 0.20:
                mid = [("=", m // 2), ("N", r.randrange(w, 6 * w)), ("X", 1), ("M", m - m // 2 - 1)]
            x["cigar"] = [c for c in x["cigar"] if c[0] in "HS"][:2] + mid
            if x["mapq"] < 15:                                                   # (no mapq test in this chain)
                x["flag"] = 0x203
            if x["flag"] & 0x800:
                x["flag"] = 0x103 if r.random() < 0.5 else 0x803
    if interleave:
        out, lists = [], [v for _k, v in sorted(by.items())]
        while lists:
            lists = [v for v in lists if v]
            for v in lists:
                out.append(v.pop())
        recs = out
    return refs, recs


def waves_with_two_refs(records):
    refs = [x["ref"] for x in records]
    waves = [refs[k:k + 64] for k in range(0, len(refs), 64)]
    return sum(1 for v in waves if len(set(v)) > 1) / float(len(waves))


def geometry(mapped, lengths, w):
    """Shares of the mapped reads that cross a window boundary, span three or more windows, are clipped by the reference's end."""
    cross = three = clipped = 0
    for ref, pos, alen in mapped:
        L = lengths[ref]
        e = min(pos + alen, L)
        clipped += pos < L and pos + alen > L
        if e > pos:
            k0, k1 = pos // w, (e - 1) // w
            cross += k1 > k0
            three += k1 - k0 >= 2
    n = float(len(mapped))
    return cross / n, three / n, clipped / n


def materialise(case, d, **bgzf):
    path = os.path.join(d, case["file"])
    sbam.write_bam(path, case["refs"], case["records"], index=case.get("index", True), **bgzf)
    return path


def params_of(case):
    p = case["params"]
    return (p["bAllReads"], p["minAlignPer"], p["maxEditDistPer"])


def load_golden():
    """tests/golden/covwin_cases.json with the shared record lists put back into the cases that name them."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covwin_cases.json")) as f:
        gold = json.load(f)
    for c in gold["cases"]:
        if isinstance(c["records"], str):
            c["records"] = gold["record_lists"][c["records"]]
    return gold
