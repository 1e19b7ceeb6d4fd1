"""TEST INFRASTRUCTURE: `checkm coverage` restated in plain Python -- the BAM reader of tests/shim/pysam.py plus the elif chain of
checkm/coverage.py:209-230 -- and what the coverage tests share: materialising a case of tests/golden/coverage_cases.json into files,
and the synthetic record generator of the structure tests.  tests/test_coverage_host.py pins the restatement to the goldens, which
the reference's own Coverage wrote on the same shim (tools/gen_coverage_golden.py)."""
import json
import os

import numpy as np

from synthdata import bam as sbam
from tests.shim import pysam as shim

SLOTS = ("reads", "duplicates", "secondary", "failed_qc", "failed_align_len", "failed_edit_dist", "failed_proper_pair", "mapped", "numerator")


def classify(read, bAllReads, minAlignPer, maxEditDistPer, minQC):
    """(class 0..7, aligned length) of one read of the shim: the reference's chain, in its order."""
    if read.is_unmapped:
        return 0, 0
    elif read.is_duplicate:
        return 1, 0
    elif read.is_secondary or read.is_supplementary:
        return 2, 0
    elif read.is_qcfail or read.mapping_quality < minQC:
        return 3, 0
    elif read.query_alignment_length < minAlignPer * read.query_length:
        return 4, 0
    elif read.get_tag('NM') > maxEditDistPer * read.query_length:
        return 5, 0
    elif not bAllReads and not read.is_proper_pair:
        return 6, 0
    return 7, read.query_alignment_length


def counters(path, bAllReads, minAlignPer, maxEditDistPer, minQC, classes=None):
    """(references, lengths, [n_ref, 9] int64) of a BAM file; `classes` (a list) receives the class of every record with a reference."""
    f = shim.Samfile(path, 'rb')
    out = np.zeros((len(f.references), 9), dtype=np.int64)
    for r in f._reads:
        if r.reference_id < 0:
            continue
        c, alen = classify(r, bAllReads, minAlignPer, maxEditDistPer, minQC)
        if classes is not None:
            classes.append(c)
        out[r.reference_id, 0] += 1
        if c:
            out[r.reference_id, c] += 1
        out[r.reference_id, 8] += alen
    return list(f.references), list(f.lengths), out


def summary(totals):
    reads = int(totals[0])
    if not reads:
        return None
    rows = (('properly mapped reads', 7), ('duplicate reads', 1), ('secondary reads', 2), ('reads failing QC', 3), ('reads failing alignment length', 4),
            ('reads failing edit distance', 5), ('reads not properly paired', 6))
    return '\n    # total reads: %d\n' % reads + ''.join('      # %s: %d (%.1f%%)\n' % (n, totals[k], float(totals[k]) * 100 / reads) for n, k in rows) + '\n'


def bin_id(path):
    return os.path.splitext(os.path.basename(path))[0]


def run(binSeqs, bamFiles, params):
    """(coverage file text, [summary per BAM]) -- binSeqs: [(bin file, [(seqId, length)])] -- rows in the reference's one-thread order."""
    to_bin, to_len = {}, {}
    for path, seqs in binSeqs:
        for seqId, n in seqs:
            to_bin[seqId], to_len[seqId] = bin_id(path), n
    info, sums = {}, []
    for path in bamFiles:
        refs, lens, cnt = counters(path, *params)
        info[path] = {}
        for k, (name, n) in enumerate(zip(refs, lens)):
            info[path][name] = (n, float(int(cnt[k, 8])) / n, int(cnt[k, 7]))
        sums.append(summary(cnt.sum(axis=0)) if len(refs) else None)
    for path in info:
        for name, st in info[path].items():
            to_len[name] = st[0]
    text = 'Sequence Id\tBin Id\tSequence length (bp)' + '\tBam Id\tCoverage\tMapped reads' * len(bamFiles) + '\n'
    for seqId, n in to_len.items():
        text += seqId + '\t' + to_bin.get(seqId, 'unbinned') + '\t' + str(n)
        for path in bamFiles:
            st = info[path].get(seqId, (0, 0, 0))
            text += '\t%s\t%f\t%d' % (bin_id(path), st[1], st[2])
        text += '\n'
    return text, sums


def materialise(case, d, **bgzf):
    """Writes the bins and the BAM files of a golden case into directory d: (bin files, BAM files, [(bin file, [(seqId, length)])])."""
    binFiles, binSeqs = [], []
    for b in case["bins"]:
        path = os.path.join(d, b["file"])
        with open(path, "w") as f:
            for seqId, n in b["seqs"]:
                f.write(">%s\n%s\n" % (seqId, ("ACGT" * (n // 4 + 1))[:n]))
        binFiles.append(path)
        binSeqs.append((path, [(s, n) for s, n in b["seqs"]]))
    bamFiles = []
    for b in case["bams"]:
        path = os.path.join(d, b["file"])
        sbam.write_bam(path, b["refs"], b["records"], index=b.get("index", True), **bgzf)
        bamFiles.append(path)
    return binFiles, bamFiles, binSeqs


def params_of(case):
    p = case["params"]
    return (p["bAllReads"], p["minAlignPer"], p["maxEditDistPer"], p["minQC"])


synthetic, PARAMS = sbam.synthetic, sbam.PARAMS


def waves_with_two_refs(records):
    """Share of the wavefronts (64 consecutive records with a reference... as the kernel sees them: 64 consecutive records) that hold two
    or more references."""
    refs = [x["ref"] for x in records]
    waves = [refs[k:k + 64] for k in range(0, len(refs), 64)]
    return sum(1 for w in waves if len(set(w)) > 1) / float(len(waves))


def load_golden():
    """tests/golden/coverage_cases.json with the shared record lists put back into the cases that name them."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage_cases.json")) as f:
        gold = json.load(f)
    for c in gold["cases"]:
        for b in c["bams"]:
            if isinstance(b["records"], str):
                b["records"] = gold["record_lists"][b["records"]]
    return gold


QA_BINS = ["binB", "binA"]


def qa_bin_stats(k):
    return {"Genome size": 2000000 + 17 * k, "# ambiguous bases": 3 * k, "# scaffolds": 40 + k, "# contigs": 44 + k, "N50 (scaffolds)": 81234 + k,
            "N50 (contigs)": 70001, "Mean scaffold length": 50000.6 + k, "Mean contig length": 45454.5, "Longest scaffold": 300123,
            "Longest contig": 250321, "GC": 0.51234 + 0.01 * k, "GC std": 0.02345, "Coding density": 0.9012, "Translation table": 11,
            "# predicted genes": 1987 + k}


def qa_parser(ns, rcase, work):
    """(ResultsParser with the two bins of the qa golden parsed from a table of reduce_cases.json, their marker sets) built from the
    classes in `ns` (HmmModel, MarkerSet, BinMarkerSets, ResultsManager, ResultsParser, DefaultValues): the reference's or the package's."""
    models = {}
    for m in rcase["models"]:
        hm = ns.HmmModel({"name": m["name"], "acc": m["acc"], "leng": m["leng"]})
        hm.ga = tuple(m["ga"]) if m["ga"] else None
        hm.tc = tuple(m["tc"]) if m["tc"] else None
        hm.nc = tuple(m["nc"]) if m["nc"] else None
        models[m["acc"]] = hm
    rp = ns.ResultsParser({b: models for b in QA_BINS})
    bms = {}
    for k, b in enumerate(QA_BINS):
        rm = ns.ResultsManager(b, models, False, ns.DefaultValues.E_VAL, ns.DefaultValues.LENGTH, False, qa_bin_stats(k))
        t = os.path.join(work, b + ".txt")
        with open(t, "w") as f:
            f.write(rcase["domtblout"])
        rp.parseHmmerResults(t, rm, k == 1)
        rp.results[b] = rm
        s = ns.BinMarkerSets(b, ns.BinMarkerSets.TAXONOMIC_MARKER_SET)
        s.addMarkerSet(ns.MarkerSet(7 + k, "k__Bacteria;p__Test", 100 + k, [set(x) for x in rcase["marker_sets"]]))
        bms[b] = s
    return rp, bms
