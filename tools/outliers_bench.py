#!/usr/bin/env python
"""Timing of the device outlier pass (checkm_amd/binTools.py BinTools.identifyOutliers).  Prints one JSON line: the wall time of one
identifyOutliers call over --bins synthetic bins (synthdata/synth_genome.py, --contigs contigs of about --contig-kb kilobases each, genes
fabricated to cover 80-95 % of a contig) against fabricated reference distributions, split as BinTools.last_timing splits it: read,
profile parse, nucleotide pass, genes, gather, upload, each kernel (seq, binsig, td, flags), host and write; binsig_gbs / td_gbs = the
bytes of the [sequences, 136] float64 rows over the kernel's time.  There is no pass/fail threshold.
usage: python tools/outliers_bench.py [--bins 64] [--contigs 400] [--contig-kb 10]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0        # MI355X peak HBM3E bandwidth (8 TB/s)

LENGTHS = [500, 1000, 2000, 5000, 10000, 20000, 50000, 100000]
PCT = [0, 0.5, 2.5, 5, 50, 95, 97.5, 99.5, 100]
Z = {0: -3.2, 0.5: -2.6, 2.5: -2.0, 5: -1.65, 50: 0.0, 95: 1.65, 97.5: 2.0, 99.5: 2.6, 100: 3.2}


def write_distributions(root):
    d = os.path.join(root, "distributions")
    os.makedirs(d)
    gc = {m / 10.0: {n: {p: Z[p] * 0.03 * (1000.0 / n) ** 0.5 for p in PCT} for n in LENGTHS} for m in range(2, 9)}
    cd = {m / 10.0: {n: {p: Z[p] * 0.06 * (1000.0 / n) ** 0.5 for p in PCT} for n in LENGTHS} for m in range(5, 10)}
    td = {n: {p: (0.05 + 0.4 * (1000.0 / n) ** 0.5) * (0.55 + p / 200.0) for p in PCT} for n in LENGTHS}
    for name, v in (("gc_dist", gc), ("cd_dist", cd), ("td_dist", td)):
        open(os.path.join(d, name + ".txt"), "w").write(repr(v))


def make_bins(work, out, n, contigs, contig_kb):
    from synthdata import synth_genome
    r = random.Random(1)
    paths = []
    with open(os.path.join(work, "assembly.fna"), "wb") as asm:
        for k in range(n):
            cs = synth_genome.make_genome(3000 + k, n_contigs=contigs, contig_len=(contig_kb * 900, contig_kb * 1100), n_runs=1)
            cs = [("b%04d_%s" % (k, cid), s) for cid, s in cs]            # ids are unique over the assembly, as a profile needs them
            p = os.path.join(work, "bin%04d.fna" % k)
            synth_genome.write_fasta(p, cs)
            asm.write(open(p, "rb").read())
            paths.append(p)
            d = os.path.join(out, "bins", "bin%04d" % k)
            os.makedirs(d)
            with open(os.path.join(d, "genes.gff"), "w") as g:
                g.write("##gff-version  3\n")
                for line in open(p):
                    if line[0] == '>':
                        cid, pos, cover = line[1:].split()[0], 1, r.uniform(0.8, 0.95)
                        while pos < contig_kb * 900 - 1200:
                            z = pos + r.randrange(300, 1200)
                            g.write("%s\tx\tCDS\t%d\t%d\t1.0\t+\t0\tID=g\n" % (cid, pos, z))
                            pos = z + 1 + int((z - pos) * (1 - cover) / cover)
    return paths, os.path.join(work, "assembly.fna")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--contigs", type=int, default=400)
    ap.add_argument("--contig-kb", type=int, default=10)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="ckm_outliers_bench_")
    out = os.path.join(work, "out")
    from checkm_amd import runtime
    from checkm_amd.binTools import BinTools
    from checkm_amd.defaultValues import DefaultValues
    from checkm_amd.genomicSignatures import GenomicSignatures
    write_distributions(work)
    DefaultValues.set_data_root(work)
    runtime.get_ctx()
    t0 = time.perf_counter()
    paths, asm = make_bins(work, out, a.bins, a.contigs, a.contig_kb)
    prof = os.path.join(work, "tetra.tsv")
    GenomicSignatures(4, 16).calculate(asm, prof)
    res = dict(bins=a.bins, contigs_per_bin=a.contigs, contig_kb=a.contig_kb, profile_bytes=os.path.getsize(prof), setup_s=round(time.perf_counter() - t0, 3))
    for rep in ("first", "second"):
        b = BinTools(16)
        ts = time.perf_counter()
        b.identifyOutliers(out, paths, prof, 95, "any", os.path.join(work, "outliers.tsv"))
        wall = time.perf_counter() - ts
        t = b.last_timing
        row_bytes = t["sequences"] * 136 * 8
        res[rep] = dict(wall_s=round(wall, 4), sequences=t["sequences"], flagged=t["flagged"],
                        **{k + "_s": round(t[k], 6) for k in ("read", "profile", "nucstats", "genes", "gather", "upload", "seq", "binsig", "td", "flags", "host", "write")},
                        binsig_gbs=round(row_bytes / max(t["binsig"], 1e-9) / 1e9, 1), td_gbs=round(row_bytes / max(t["td"], 1e-9) / 1e9, 1))
    res["hbm_gbs"] = HBM_GBS
    print(json.dumps(res))
    if os.environ.get("CKM_BENCH_OUT"):
        with open(os.environ["CKM_BENCH_OUT"], "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
