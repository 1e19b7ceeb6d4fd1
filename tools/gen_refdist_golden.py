#!/usr/bin/env python
"""Goldens of ReferenceDistributions: the reference's own GenomicSignatures(4, 1).seqSignature / distance,
ProdigalGeneFeatureParser.codingBases and readFasta (imported from a CheckM source tree named by CHECKM_SOURCE) and numpy, driven
through the loops DESIGN §18 states for scripts/distributionDelta*.py and calculateBounds*.py (the scripts themselves are Python 2 and
cannot run).  Only data is recorded: input texts, parameters, every float as float.hex(), the texts of the per-genome and bounds files;
failures by type and args.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_refdist_golden.py > tests/golden/refdist_cases.json
       CHECKM_SOURCE=<checkm source> python tools/gen_refdist_golden.py --time --mb N    (times the reference's TD sampling loop on one
                                                                          core, writes profiles/r14_refdist_reference_cpu.json)"""
import contextlib
import json
import os
import random
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = {"gc": "", "td": "NNNN", "cd": "N" * 10}
MODEL = "# Sequence Data: seqnum=1;seqlen=100;seqhdr=\"x\"\n# Model Data: version=Prodigal.v2.6.3;run_type=Single;model=\"Ab initio\";gc_cont=50.00;transl_table=11;uses_sd=1\n"
CAP = 5


def rnd(r, n, chars="ACGT"):
    return "".join(r.choice(chars) for _ in range(n))


def sprinkle(r, s, chars, n):
    s = list(s)
    for _ in range(n):
        s[r.randrange(len(s))] = r.choice(chars)
    return "".join(s)


def fasta(pairs, width=60):
    return "".join(">%s\n%s" % (k, "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))) for k, s in pairs)


def gene_rows(cid, spans):
    return "".join("%s\tProdigal_v2.6.3\tCDS\t%d\t%d\t10.0\t+\t0\tID=1_%d;partial=00\n" % (cid, a, z, k + 1) for k, (a, z) in enumerate(spans))


def build_cases():
    r = random.Random(20261018)
    cases = []
    mixed = [("m0", sprinkle(r, rnd(r, 140), "acgtUuRY", 14)), ("m1", rnd(r, 20) + "N" * 15 + rnd(r, 30).lower()), ("m2", rnd(r, 41).replace("T", "U"))]
    Lgc = sum(len(s) for _, s in mixed)
    cases.append(dict(name="mixed", fasta=fasta(mixed), gff=None, stats=["gc", "td"], numWindows=12, seed=7,
                      sizes=[1, 3, 4, 5, 10, 16, 17, 40, 100, Lgc - 1, Lgc, Lgc + 7, Lgc + 8, Lgc + 9, 500]))
    genes = [("g0", rnd(r, 150)), ("g1", rnd(r, 80).lower()), ("g2", rnd(r, 64).replace("T", "U")), ("g3", rnd(r, 33)), ("g4", rnd(r, 7))]
    # in coordinates of the ten-N scaffold (g0 1-150, g1 161-240, g2 251-314, g3 325-357, g4 368-374): overlapping, nested, across joins
    gff = "##gff-version  3\n" + MODEL + gene_rows("genes", [(5, 60), (40, 100), (50, 55), (120, 170), (200, 260), (300, 340), (330, 336), (370, 374)]) + gene_rows("other", [(1, 50)])
    cases.append(dict(name="genes", fasta=fasta(genes), gff=gff, stats=["gc", "cd", "td"], numWindows=15, seed=0, sizes=[1, 4, 5, 10, 11, 32, 60, 64]))
    cases.append(dict(name="cd_never", fasta=fasta(genes), gff=gff, stats=["cd"], numWindows=3, seed=1, sizes=[10, 151, 200]))
    cases.append(dict(name="nogenes", fasta=fasta(genes[:2]), gff="##gff-version  3\n" + MODEL + gene_rows("other", [(1, 50)]), stats=["cd"], numWindows=5, seed=2, sizes=[7, 30]))
    single = [("only", rnd(r, 60))]
    cases.append(dict(name="single", fasta=fasta(single), gff="##gff-version  3\n" + MODEL + gene_rows("single", [(3, 20), (30, 58)]), stats=["gc", "cd", "td"], numWindows=9, seed="s",
                      sizes=[1, 2, 3, 4, 7, 59, 60, 61]))
    cases.append(dict(name="t10", fasta=">t\nNNACGTACGTAN\n", gff=None, stats=["gc"], numWindows=40, seed=3, sizes=[10]))
    cases.append(dict(name="t500", fasta=fasta([("t", "N" * 51 + rnd(r, 449) + "A")]), gff=None, stats=["gc"], numWindows=20, seed=4, sizes=[500]))
    cases.append(dict(name="gc_never", fasta=">n\n" + "N" * 30 + "ACGT\n", gff=None, stats=["gc"], numWindows=3, seed=5, sizes=[4, 20, 25]))
    cases.append(dict(name="empty", fasta="", gff="##gff-version  3\n", stats=["gc", "cd", "td"], numWindows=2, seed=0, sizes=[1, 4]))
    return cases


def hexes(v):
    return [float(x).hex() for x in v]


def sample(L, sizes, numWindows, seed, genomeId, stat, value):
    out = {}
    for w in sizes:
        if L - w <= 0:
            break
        rng, vals, draws = random.Random("%s:%s:%s:%d" % (seed, genomeId, stat, w)), [], 0
        while len(vals) != numWindows:
            if draws == 100 * numWindows:
                raise ValueError(genomeId, stat, w)
            s = rng.randint(0, L - w)
            draws += 1
            v = value(s, w)
            if v is not None:
                vals.append(v)
        out[w] = vals
    return out


def file_text(stat, head, dist):
    text = "# Tetra signature = " + ",".join(str(float(v)) for v in head) + "\n" if stat == "td" else "# Mean %s = %s\n" % (stat.upper(), str(float(head)))
    for w, vals in dist.items():
        text += "Windows Size = " + str(w) + "\n" + ",".join(str(float(v)) for v in vals) + "\n"
    return text


def classes(s):
    return s.count("C") + s.count("G"), s.count("A") + s.count("T") + s.count("U")


def one(stat, c, seqs, gffPath, gs, Parser):
    genomeId, n, sizes, seed = c["name"], c["numWindows"], c["sizes"], c["seed"]
    scaf = SEP[stat].join(seqs.values())
    if stat != "td":
        scaf = scaf.upper()
    if stat == "gc":
        gc, at = classes(scaf)
        head = float(gc) / (gc + at)

        def value(s, w):
            g, a = classes(scaf[s:s + w])
            return None if g + a < 0.9 * w else float(g) / (g + a) - head
    elif stat == "cd":
        parser = Parser(gffPath)
        gc, at = classes(scaf)
        head = float(parser.codingBases(genomeId)) / (gc + at)

        def value(s, w):
            g, a = classes(scaf[s:s + w])
            return None if g + a != w else float(parser.codingBases(genomeId, s, s + w)) / (g + a) - head
    else:
        head = gs.seqSignature(scaf)

        def value(s, w):
            return gs.distance(head, gs.seqSignature(scaf[s:s + w]))
    return head, sample(len(scaf), sizes, n, seed, genomeId, stat, value)


CIS = np.arange(0, 100 + 0.5, 0.5).tolist()


def percentiles(pts):
    return {ci: float(p) for ci, p in zip(CIS, np.percentile(np.array(pts), CIS))}


def windows_of(text):
    out, w = [], None
    for line in text.splitlines():
        if "Windows Size" in line:
            w = int(line.split("=")[1].strip())
        elif w is not None:
            out.append((w, line))
            w = None
    return out


def bounds_case(r):
    means = dict(a=0.285, b=0.3, c=0.315, d=0.31, e=0.7, f=0.52, g=0.53)
    files = {g: file_text("gc", m, {500: [r.uniform(-0.1, 0.1) for _ in range(7)], 600: [r.uniform(-0.05, 0.05) for _ in range(4)]}) for g, m in means.items()}
    p = dict(stepSize=0.01, width=0.015, minGenomes=2)
    out = {}
    for centre in np.arange(0.0, 1.0 + 0.5 * p["stepSize"], p["stepSize"]):
        ids = [g for g in sorted(files) if means[g] >= centre - p["width"] and means[g] <= centre + p["width"]]
        if len(ids) < p["minGenomes"]:
            continue
        d = {}
        for g in ids:
            for w, line in windows_of(files[g]):
                d.setdefault(w, []).extend(float(x) for x in line.split(","))
        out[float(centre)] = {w: percentiles(pts) for w, pts in d.items()}
    assert 0.3 in out and not any(abs(k - 0.7) < 0.02 for k in out)
    return dict(files=files, params=p, text=str(out), centres=hexes(out.keys()))


def bounds_td_case(r):
    sig = [1.0 / 136] * 136
    files = dict(x=file_text("td", sig, {500: [r.random() for _ in range(8)], 600: [r.random() for _ in range(3)]}),
                 y=file_text("td", sig, {500: [r.random(), float("nan"), r.random()], 600: [r.random() for _ in range(5)]}),
                 z=file_text("td", sig, {500: [r.random() for _ in range(4)], 700: [r.random() for _ in range(6)]}))
    windows, bad, seed = {}, [], 11
    for g in sorted(files):
        for w, line in windows_of(files[g]):
            if "nan" in line:
                bad.append(g)
                continue
            vals = [float(x) for x in line.split(",")]
            if len(vals) > CAP:
                vals = random.Random("%s:%s:%d" % (seed, g, w)).sample(vals, CAP)
            windows.setdefault(w, []).extend(vals)
    out = {w: percentiles(pts) for w, pts in windows.items()}
    return dict(files=files, seed=seed, cap=CAP, text=str(out), bad=bad)


def main():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    os.environ.setdefault("CHECKM_DATA_PATH", tempfile.mkdtemp(prefix="ckm_refdist_data_"))
    with contextlib.redirect_stdout(sys.stderr):               # the package reports its data folder on import
        from checkm.genomicSignatures import GenomicSignatures
        from checkm.prodigal import ProdigalGeneFeatureParser
        from checkm.util.seqUtils import readFasta
    gs = GenomicSignatures(4, 1)
    if "--time" in sys.argv:
        return time_reference(gs, int(sys.argv[sys.argv.index("--mb") + 1]))
    work = tempfile.mkdtemp(prefix="ckm_refdist_gold_")
    result = dict(cases=[])
    seen = set()
    for c in build_cases():
        path, gffPath = os.path.join(work, c["name"] + ".fna"), os.path.join(work, c["name"] + ".gff")
        open(path, "w").write(c["fasta"])
        if c["gff"] is not None:
            open(gffPath, "w").write(c["gff"])
        seqs = readFasta(path)
        c["scaffold_file"] = ">" + c["name"] + "\n" + SEP["cd"].join(seqs.values()).upper()
        c["results"] = {}
        for stat in c["stats"]:
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    head, dist = one(stat, c, seqs, gffPath, gs, ProdigalGeneFeatureParser)
                res = dict(error=None, head=hexes(head) if stat == "td" else float(head).hex(), dist={str(w): hexes(v) for w, v in dist.items()}, file=file_text(stat, head, dist))
                if any("nan" in v for v in res["dist"].values()):
                    seen.add("nan")
                if len(dist) < len(c["sizes"]):
                    seen.add("dropped")
            except (ValueError, ZeroDivisionError) as e:
                res = dict(error=dict(type=type(e).__name__, args=[str(a) for a in e.args]))
                seen.add((stat, type(e).__name__))
            c["results"][stat] = res
        result["cases"].append(c)
    for need in ("nan", "dropped", ("gc", "ValueError"), ("cd", "ValueError"), ("gc", "ZeroDivisionError"), ("cd", "ZeroDivisionError")):
        assert need in seen, (need, sorted(map(str, seen)))
    r = random.Random(5)
    result["bounds"] = bounds_case(r)
    result["boundsTD"] = bounds_td_case(r)
    json.dump(result, sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")


def time_reference(gs, mb):
    """The TD sampling loop of distributionDeltaTetraDiff.py on one core: seqSignature of random windows and their distance, a few per size."""
    r = random.Random(1)
    seq = "".join(r.choice("ACGT") for _ in range(mb << 20))
    genomeSig = gs.seqSignature(seq[:100000])
    sizes, per = [500, 5000, 50000], 20
    t0 = time.perf_counter()
    bases = 0
    for w in sizes:
        for _ in range(per):
            s = r.randint(0, len(seq) - w)
            gs.distance(genomeSig, gs.seqSignature(seq[s:s + w]))
            bases += w
    dt = time.perf_counter() - t0
    out = dict(what="reference TD sampling loop (seqSignature + distance per random window), one core", megabytes=mb, sizes=sizes, windows_per_size=per, window_bases=bases,
               seconds=dt, seconds_per_1e9_window_bases=dt * 1e9 / bases, numpy=np.__version__)
    open(os.path.join(ROOT, "profiles", "r14_refdist_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
