#!/usr/bin/env python
"""Goldens of the bin-statistics and tetranucleotide contract produced by the REFERENCE's own classes (checkm/binStatistics.py,
checkm/genomicSignatures.py, checkm/util/seqUtils.py readFasta imported from a CheckM source tree on PYTHONPATH): for every case the
input texts (FASTA, genes.gff, genes.faa), readFasta's view and the line BinStatistics.calculate writes (None when its worker dies), and
for the tetra cases the whole file GenomicSignatures.calculate writes.  Every bin is computed by a calculate() call of its own, so that a
bin whose worker dies takes no other bin with it.
usage: PYTHONPATH=<checkm source> python tools/gen_nucstats_golden.py > tests/golden/nucstats_cases.json"""
import gzip
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = tempfile.mkdtemp(prefix="ckm_data_")          # the reference wants a data root at import time (checkm/checkmData.py:115-121)
os.makedirs(os.path.join(DATA, "pfam"))
open(os.path.join(DATA, "pfam", "Pfam-A.hmm.dat"), "w").close()
os.environ["CHECKM_DATA_PATH"] = DATA

# cases whose tetra file is recorded too: the reader rules, the alphabet, runs of 'N' and rows without a valid window
TETRA_CASES = ("crlf", "no_final_newline", "duplicate_id", "gzip", "n_runs", "alphabet", "short_and_cutoff", "utf8", "no_contig_base")
MODEL = '# Model Data: version=Prodigal.v2.6.3;run_type=Single;model="Ab initio";gc_cont=50.00;transl_table=%d;uses_sd=1\n'


def rnd(r, n, alphabet="ACGT"):
    return "".join(r.choice(alphabet) for _ in range(n))


def wrap(s, w=60, eol="\n"):
    return "".join(s[i:i + w] + eol for i in range(0, len(s), w))


def gff_faa(r, contigs, table=11, extra_ids=()):
    gff, faa = ["##gff-version  3\n", "# Sequence Data: seqnum=1;seqlen=1;seqhdr=\"x\"\n", MODEL % table], []
    for cid, n in list(contigs) + [(e, 600) for e in extra_ids]:
        k = 0
        pos = 1
        while pos + 90 < n:
            a = pos + r.randrange(0, 60)
            b = min(n, a + r.randrange(90, 900))
            k += 1
            gff.append("%s\tProdigal_v2.6.3\tCDS\t%d\t%d\t10.0\t%s\t0\tID=1_%d;partial=00\n" % (cid, a, b, r.choice("+-"), k))
            faa.append(">%s_%d # %d # %d # 1\nM%s*\n" % (cid, k, a, b, rnd(r, (b - a) // 3 - 1, "ACDEFGHIKLMNPQRSTVWY")))
            pos = max(1, a + r.randrange(-50, 400)) if r.random() < 0.3 else b + r.randrange(1, 200)   # overlaps; prodigal never starts below 1
    return "".join(gff), "".join(faa)


def cases():
    r = random.Random(20261016)
    out = []

    def add(name, fasta, genes=True, gz=False, extra_ids=(), table=11):
        out.append(dict(name=name, fasta=fasta, gz=gz, genes=genes, extra_ids=list(extra_ids), table=table))

    s1, s2 = rnd(r, 300), rnd(r, 180)
    add("crlf", ">c1 first contig\r\n" + wrap(s1, 70, "\r\n") + ">c2\r\n" + wrap(s2.lower(), 50, "\r\n") + "\r\n")
    add("lone_cr", ">c1\r" + wrap(rnd(r, 250), 60, "\r") + ">c2 x\r" + rnd(r, 300))
    add("no_final_newline", ">a\n" + wrap(rnd(r, 260)) + ">b desc\nACGTACGTACGTU")
    add("blanks_tabs", ">a\n" + "AC GT\tAC\n  \n\t\n" + wrap(rnd(r, 220)) + "GGCC  \n>b\n \tACGT ACGT\n")
    add("duplicate_id", ">a\n" + wrap(rnd(r, 280)) + ">b\n" + wrap(rnd(r, 190)) + ">a second\n" + wrap(rnd(r, 330)))
    add("gzip", ">g1\n" + wrap(rnd(r, 1150)) + ">g2\n" + wrap(rnd(r, 1020)), gz=True)
    runs = [9, 10, 11, 20, 25]
    seqs = []
    for n in runs:
        seqs.append(">run%d\n%s\n" % (n, "N" * n + rnd(r, 40) + "N" * n + rnd(r, 30) + "N" * n))
    seqs.append(">mixed\n%s\n" % (rnd(r, 50) + "N" * 9 + "n" * 3 + "N" * 7 + rnd(r, 60) + "NNNNNNNNNnNNNNN" + rnd(r, 20)))
    add("n_runs", "".join(seqs))
    add("alphabet", ">allN\n" + "N" * 37 + "\n>lower_n\nnnnnacgtacgtnnnnnnnnnnnnacgt\n>with_u\nACGUUUGCAuuu\n>iupac\nACGTRYKMSWBDHVNacgtrykmswbdhvn\n"
        ">acgt\n" + wrap(rnd(r, 150, "acgt")))
    add("short_and_cutoff", ">s1\nA\n>s2\nAC\n>s3\nACG\n>e1000\n" + wrap(rnd(r, 1000)) + ">e1001\n" + wrap(rnd(r, 1001)) + ">e1002\n" + wrap(rnd(r, 1002, "GGGCCA")) +
        ">e999\n" + wrap(rnd(r, 999, "AT")))
    add("no_gff", ">x\n" + wrap(rnd(r, 300)) + ">y\n" + wrap(rnd(r, 200)), genes=False)
    add("gff_foreign_ids", ">p\n" + wrap(rnd(r, 700)) + ">q\n" + wrap(rnd(r, 500)), extra_ids=("not_here", "other"), table=4)
    add("utf8", ">u1 é\n" + wrap(rnd(r, 200)) + "ACGTéNNNNNNNNNNNéACG\n>u2\nACGTAé")
    add("no_contig_base", ">a\n" + "N" * 30 + "\n>b\n\n>c\nNNNNNNNNNNNNNNNNNNNN\n")
    return out


def main():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    from checkm.binStatistics import BinStatistics
    from checkm.genomicSignatures import GenomicSignatures
    from checkm.util.seqUtils import readFasta
    r = random.Random(7)
    work = tempfile.mkdtemp(prefix="ckm_nucstats_gold_")
    result = dict(bins=[], tetra=[])
    for c in cases():
        d = os.path.join(work, c["name"])
        os.makedirs(os.path.join(d, "out", "storage"))
        path = os.path.join(d, c["name"] + (".fna.gz" if c["gz"] else ".fna"))
        data = c["fasta"].encode("utf-8")
        if c["gz"]:
            with gzip.open(path, "wb") as f:
                f.write(data)
        else:
            open(path, "wb").write(data)
        view = readFasta(path)
        gff = faa = None
        if c["genes"]:
            gff, faa = gff_faa(r, [(k, len(v)) for k, v in view.items()], c["table"], c["extra_ids"])
            bdir = os.path.join(d, "out", "bins", c["name"])
            os.makedirs(bdir)
            open(os.path.join(bdir, "genes.gff"), "w").write(gff)
            open(os.path.join(bdir, "genes.faa"), "w").write(faa)
        BinStatistics(1).calculate([path], os.path.join(d, "out"), "bin_stats.tsv")
        line = open(os.path.join(d, "out", "storage", "bin_stats.tsv")).read()
        result["bins"].append(dict(name=c["name"], fasta=c["fasta"], gz=c["gz"], gff=gff, faa=faa, view=[[k, v] for k, v in view.items()],
                                   line=line if line else None))
        if c["name"] in TETRA_CASES:
            tet = os.path.join(d, "tetra.tsv")
            GenomicSignatures(4, 1).calculate(path, tet)
            result["tetra"].append(dict(name=c["name"], text=open(tet).read()))
    json.dump(result, sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
