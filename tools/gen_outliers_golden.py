#!/usr/bin/env python
"""Goldens of `checkm outliers`, `modify` and `unique` produced by the REFERENCE's own BinTools (checkm/binTools.py imported from a CheckM
source tree named by CHECKM_SOURCE): fabricated reference distributions, bins with planted outliers, their genes.gff, a tetranucleotide
profile written by the reference's GenomicSignatures.calculate, and the file identifyOutliers writes for every distribution in
{90, 95, 99} x reportType in {'any', 'all'}; the files modify / removeOutliers write and what unique prints.

Only data is recorded: input texts, the distributions, the reference's outputs.  The tetranucleotide profile itself (2.7 kB per sequence)
is not stored: the fixture holds the FASTA text it was computed from, the rows appended to it (a repeated id) and the SHA-256 of the
whole file, and the tests rebuild it through the writer that tests/golden/nucstats_cases.json pins to the reference's.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_outliers_golden.py > tests/golden/outliers_cases.json"""
import contextlib
import hashlib
import io
import json
import logging
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = tempfile.mkdtemp(prefix="ckm_data_")          # the reference wants a data root at import time (checkm/checkmData.py:115-121)
os.makedirs(os.path.join(DATA, "pfam"))
os.makedirs(os.path.join(DATA, "distributions"))
open(os.path.join(DATA, "pfam", "Pfam-A.hmm.dat"), "w").close()
os.environ["CHECKM_DATA_PATH"] = DATA

LENGTHS = [1000, 200, 400, 700, 1500, 2000, 5000, 100]       # dict order is not sorted order: the first minimum is by position
PCT = [0, 0.5, 2.5, 5, 50, 95, 97.5, 99.5, 100]
Z = {0: -3.2, 0.5: -2.6, 2.5: -2.0, 5: -1.65, 50: 0.0, 95: 1.65, 97.5: 2.0, 99.5: 2.6, 100: 3.2}
GC_MEANS = [0.5, 0.25, 0.75, 0.625]                           # 0.375 ties between 0.5 and 0.25; exactly representable, so the tie is exact
CD_MEANS = [0.9, 0.5, 0.7, 0.8]
MODEL = '# Model Data: version=Prodigal.v2.6.3;run_type=Single;model="Ab initio";gc_cont=50.00;transl_table=11;uses_sd=1\n'


def distributions():
    gc = {m: {n: {p: round(Z[p] * (0.035 + 0.02 * abs(m - 0.5)) * (1000.0 / n) ** 0.5, 4) for p in PCT} for n in LENGTHS} for m in GC_MEANS}
    cd = {m: {n: {p: round(Z[p] * (0.06 + 0.05 * (0.9 - m)) * (1000.0 / n) ** 0.5, 4) for p in PCT} for n in LENGTHS} for m in CD_MEANS}
    td = {n: {p: round((0.25 + 0.45 * (1000.0 / n) ** 0.5) * (0.55 + p / 200.0), 4) for p in PCT} for n in LENGTHS}
    return dict(gc_dist=repr(gc), cd_dist=repr(cd), td_dist=repr(td))


def rnd(r, n, gc=0.5):
    return "".join(r.choice("GC") if r.random() < gc else r.choice("AT") for _ in range(n))


def exact_gc(r, n, ngc):
    s = [r.choice("GC") for _ in range(ngc)] + [r.choice("AT") for _ in range(n - ngc)]
    r.shuffle(s)
    return "".join(s)


def wrap(s, w=70):
    return "".join(s[i:i + w] + "\n" for i in range(0, len(s), w))


def genes(r, cid, n, frac=0.9, overlap=False):
    """GFF rows covering about `frac` of a contig of n bases; with overlap, neighbouring genes share bases."""
    rows, pos, k = [], 1, 0
    while pos + 60 < n:
        a = pos
        b = min(n, a + r.randrange(90, 320))
        k += 1
        rows.append("%s\tProdigal_v2.6.3\tCDS\t%d\t%d\t10.0\t%s\t0\tID=1_%d;partial=00\n" % (cid, a, b, r.choice("+-"), k))
        gap = int((b - a) * (1 - frac) / frac) + r.randrange(0, 6)
        pos = max(1, b - r.randrange(10, 60)) if overlap and k % 2 else b + 1 + gap
    return "".join(rows)


def fasta(recs):
    return "".join(">%s\n%s" % (cid, wrap(s)) for cid, s in recs)


def build_cases():
    r = random.Random(20261016)
    cases = []
    # ---- the main case: three bins in one call -----------------------------------------------------------------------------------------
    main = [("m%02d" % k, rnd(r, n)) for k, n in enumerate([1000, 1400, 300, 850, 2000, 1200, 640, 1700, 900, 1100])]   # 300 and 850 tie between two length keys
    main[1] = (main[1][0], main[1][1].lower())
    main[4] = (main[4][0], main[4][1].replace("T", "U", 40))
    s = list(main[5][1])
    for at in range(50, 1150, 97):
        s[at] = "RYKMSWN"[at % 7]
    main[5] = (main[5][0], "".join(s))
    planted = [("gc_only", rnd(r, 1000, 0.66)), ("cd_only", rnd(r, 1000)), ("td_only", "ACGTTGCAAGCTTCGA" * 60),
               ("all_three", "GGGCGGCCGCGGGGCC" * 56 + "A" * 4), ("no_genes_short", rnd(r, 240))]
    no_gene_ids = {"cd_only", "all_three", "no_genes_short", "m02", "m03"}          # m02 and m03: flagged, so their tied length key shows in the row
    gff = ["##gff-version  3\n", MODEL]
    for k, (cid, s) in enumerate(main + planted):
        if cid not in no_gene_ids:
            gff.append(genes(r, cid, len(s), overlap=(k % 3 == 0)))
    bin_main = dict(name="main", fasta=fasta(main + planted), gff="".join(gff))
    tie = [("t0", exact_gc(r, 800, 300)), ("t1", exact_gc(r, 1600, 600)), ("t2", exact_gc(r, 400, 150)), ("t_hi", exact_gc(r, 800, 400)), ("t_lo", exact_gc(r, 800, 200))]   # 3/8 in total
    bin_tie = dict(name="tie_gc", fasta=fasta(tie), gff="##gff-version  3\n" + MODEL + "".join(genes(r, c, len(s), 0.7) for c, s in tie))
    nanb = [("n0", rnd(r, 900)), ("n1", rnd(r, 1300)), ("nowin", "ACGNNACNNGT"), ("n_motif", "ACGTTGCAAGCTTCGA" * 50), ("n_gc", rnd(r, 1000, 0.7))]
    bin_nan = dict(name="nan_bin", fasta=fasta(nanb), gff="##gff-version  3\n" + MODEL + "".join(genes(r, c, len(s)) for c, s in nanb if c != "nowin"))
    extra = [("x_unbinned1", rnd(r, 500)), ("x_unbinned2", rnd(r, 350, 0.4))]
    cases.append(dict(name="three_bins", bins=[bin_main, bin_tie, bin_nan], profile_fasta=fasta(extra[:1] + main + planted + tie + nanb + extra[1:]),
                      repeat=[["m03", "x_unbinned2"], ["x_unbinned1", "m00"]],
                      runs=[[d, t] for d in (90, 95, 99) for t in ("any", "all")]))
    # ---- the reference's failures ------------------------------------------------------------------------------------------------------
    ok = [("k0", rnd(r, 600)), ("k1", rnd(r, 700))]
    okbin = dict(name="ok", fasta=fasta(ok), gff="##gff-version  3\n" + MODEL + "".join(genes(r, c, len(s)) for c, s in ok))
    cases.append(dict(name="missing_gff", bins=[okbin, dict(name="nogff", fasta=fasta([("g0", rnd(r, 500))]), gff=None)],
                      profile_fasta=fasta(ok + [("g0", rnd(r, 500))]), repeat=[], runs=[[95, "any"]]))
    cases.append(dict(name="missing_id", bins=[okbin, dict(name="stranger", fasta=fasta([("k0", ok[0][1]), ("not_in_profile", rnd(r, 500))]),
                                                            gff="##gff-version  3\n" + MODEL + genes(r, "k0", 600))],
                      profile_fasta=fasta(ok), repeat=[], runs=[[95, "any"]]))
    cases.append(dict(name="zero_division", bins=[okbin, dict(name="onlyn", fasta=fasta([("k1", ok[1][1]), ("z0", "NNNNNNNN")]), gff="##gff-version  3\n" + MODEL)],
                      profile_fasta=fasta(ok + [("z0", "NNNNNNNN")]), repeat=[], runs=[[95, "any"]]))
    return cases


class Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.text = []

    def emit(self, record):
        self.text.append(record.getMessage())


def main():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    dist = distributions()
    for k, v in dist.items():
        open(os.path.join(DATA, "distributions", k + ".txt"), "w").write(v)
    from checkm.binTools import BinTools
    from checkm.genomicSignatures import GenomicSignatures
    cap = Capture()
    logging.getLogger("timestamp").addHandler(cap)
    work = tempfile.mkdtemp(prefix="ckm_outliers_gold_")
    result = dict(distributions=dist, cases=[], modify=[], unique=[])
    combos = set()
    for c in build_cases():
        d = os.path.join(work, c["name"])
        os.makedirs(d)
        paths = []
        for b in c["bins"]:
            p = os.path.join(d, b["name"] + ".fna")
            open(p, "w").write(b["fasta"])
            paths.append(p)
            if b["gff"] is not None:
                os.makedirs(os.path.join(d, "out", "bins", b["name"]))
                open(os.path.join(d, "out", "bins", b["name"], "genes.gff"), "w").write(b["gff"])
        pf = os.path.join(d, "profile.fna")
        open(pf, "w").write(c["profile_fasta"])
        tet = os.path.join(d, "tetra.tsv")
        GenomicSignatures(4, 1).calculate(pf, tet)
        rows = dict((ln.split("\t", 1)[0], ln.split("\t", 1)[1]) for ln in open(tet).read().splitlines(True)[1:])
        with open(tet, "a") as f:
            for seqId, source in c["repeat"]:
                f.write(seqId + "\t" + rows[source])
        c["profile_sha256"] = hashlib.sha256(open(tet, "rb").read()).hexdigest()
        runs = []
        for distribution, reportType in c["runs"]:
            out = os.path.join(d, "outliers_%d_%s.tsv" % (distribution, reportType))
            del cap.text[:]
            error = None
            try:
                BinTools().identifyOutliers(os.path.join(d, "out"), paths, tet, distribution, reportType, out)
            except SystemExit as e:
                error = dict(type="SystemExit", code=e.code, log=list(cap.text))
            except (KeyError, ZeroDivisionError) as e:
                error = dict(type=type(e).__name__, args=[str(a) for a in e.args])
            text = None if error else open(out).read()
            if text:
                for ln in text.splitlines()[1:]:
                    combos.add(ln.split("\t")[3])
            runs.append(dict(distribution=distribution, reportType=reportType, output=text, error=error))
        c["runs"] = runs
        result["cases"].append(c)
    # the fixture cannot degenerate: every kind of row is there
    for need in ("GC", "CD", "TD", "GC,CD,TD"):
        assert need in combos, (need, sorted(combos))
    three = result["cases"][0]
    assert all(any(ln.startswith(want) for ln in three["runs"][0]["output"].splitlines()) for want in ("main\tm02\t300", "main\tm03\t850", "tie_gc\tt_hi", "tie_gc\tt_lo"))
    assert not any("n_motif" in (run["output"] or "") and "TD" in ln.split("\t")[3] for run in three["runs"] for ln in run["output"].splitlines()[1:] if ln.startswith("nan_bin"))
    assert [c["runs"][0]["error"]["type"] for c in result["cases"][1:]] == ["SystemExit", "KeyError", "ZeroDivisionError"]

    # ---- modify / removeOutliers / unique ------------------------------------------------------------------------------------------------
    r = random.Random(5)
    d = os.path.join(work, "modify")
    os.makedirs(d)
    binf = ">a desc\n%s>b\n%s>c\n%s" % (wrap(rnd(r, 150), 60), wrap(rnd(r, 100).lower(), 60), wrap(rnd(r, 90), 60))
    reff = ">x\n%s>y more\n%s>a\n%s" % (wrap(rnd(r, 80), 60), wrap(rnd(r, 130), 60), wrap(rnd(r, 70), 60))
    outl = three["runs"][0]["output"].splitlines(True)[0] + "binA\tb\t100\tGC\n" + "other\tc\t90\tGC\n" + "binA\tc\t90\tTD\n"
    open(os.path.join(d, "binA.fna"), "w").write(binf)
    open(os.path.join(d, "ref.fna"), "w").write(reff)
    open(os.path.join(d, "outliers.tsv"), "w").write(outl)
    for add, rem in ((["x", "a"], ["b"]), (None, ["a", "c"]), (["y"], None), (["nope"], None), (None, ["nope", "b"])):
        out = os.path.join(d, "out.fna")
        del cap.text[:]
        error = None
        try:
            BinTools().modify(os.path.join(d, "binA.fna"), os.path.join(d, "ref.fna"), add, rem, out)
        except SystemExit as e:
            error = dict(type="SystemExit", code=e.code, log=list(cap.text))
        result["modify"].append(dict(kind="modify", bin=binf, ref=reff, add=add, remove=rem, output=None if error else open(out).read(), error=error))
    out = os.path.join(d, "out2.fna")
    BinTools().removeOutliers(os.path.join(d, "binA.fna"), os.path.join(d, "outliers.tsv"), out)
    result["modify"].append(dict(kind="removeOutliers", bin=binf, outliers=outl, output=open(out).read(), error=None))
    for files in ([("u1", ">s1\nACGT\n>s2 x\nAC\n>s1\nGG\n"), ("u2", ">s2\nAC\n>s3\nTT\n"), ("u3", ">s4\nAC\n>s3\nTT\n>s1\nA\n")],
                  [("v1", ">p\nAC\n"), ("v2", ">q\nAC\n")]):
        paths = []
        for name, text in files:
            paths.append(os.path.join(d, name + ".fna"))
            open(paths[-1], "w").write(text)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            BinTools().unique(paths)
        result["unique"].append(dict(files=[list(f) for f in files], stdout=buf.getvalue()))
    json.dump(result, sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
