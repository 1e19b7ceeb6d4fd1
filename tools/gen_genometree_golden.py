#!/usr/bin/env python
"""Goldens of GenomeTree's host part: the class of scripts/genometreeworkflow/inferGenomeTree.py (its run up to the FastTree call, with
__genesInGenomes, __filterParalogs and __taxonomy) and the column draw of scripts/genometreeworkflow/bootstrapTree.py of the reference,
with the reference's own checkm.util.img.IMG, readFasta, writeFasta and appendTaxonomyRanks, over a small synthetic genome directory.
The scripts are Python 2 and do not compile as they stand; their class text is loaded in memory after the substitutions listed below
(each counted) and never written to disk.  The scripts' surroundings are stand-ins handed to the loaded classes, not changes of their
text: `IMG` is a callable that ignores the paths of the authors' machine and returns the reference's IMG over the synthetic files (with
the class attributes the script reads), and `os` is the real module but for `system`, which records the FastTree command instead of
running it.
The taxonomy file follows the metadata file's order (a dict of the running Python keeps it); the records of the alignment follow the
order of a set of strings, which depends on the hash seed: the case says order_free = false and the test compares the records as a
sorted list.  Before anything is written the evolved 16-leaf fixture of tests/test_genometree_host.py is checked with the plain numpy
neighbour joining, as tools/gen_placement_golden.py checks its fixture.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_genometree_golden.py              (writes tests/golden/genometree_cases.json)"""
import contextlib
import io
import json
import os
import random
import re
import sys
import tempfile
import types
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_simulation_golden import translate                                                                        # noqa: E402

INFER_SUBSTITUTIONS = [("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)"),
                       ("keys() sliced as a list", r"seqs\.keys\(\)\[i\+1:\]", "list(seqs.keys())[i+1:]"),
                       ("first key of a dict", r"seqs\.keys\(\)\[0\]", "list(seqs.keys())[0]")]
INFER_HITS = {"print statements": 9, "keys() sliced as a list": 1, "first key of a dict": 1}
BOOT_SUBSTITUTIONS = [("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)"), ("xrange", r"\bxrange\(", "range("),
                      ("first key of a dict", r"seqs\.keys\(\)\[0\]", "list(seqs.keys())[0]")]
BOOT_HITS = {"print statements": 5, "xrange": 2, "first key of a dict": 1}

METADATA_HEADER = ["taxon_oid", "Domain", "Status", "Phylum", "Class", "Order", "Family", "Genus", "Species", "Scaffold Count", "GC Count", "Genome Size", "Gene Count",
                   "Coding Base Count", "Biotic Relationships", "N50"]


def pfam_line(gene, family, evalue):
    return "\t".join([gene, "300", "50.0", "1", "100", "1", evalue, "x", family, "name"]) + "\n"      # gene in column 0, the e-value the script reads in 6, family in 8


def tigr_line(gene, family, evalue):
    return "\t".join([gene, "300", "50.0", "1", evalue, "x", family, "name"]) + "\n"                                 # e-value in column 4, family in 6


def concatenate_case():
    """Five genomes, four genes with a tree (two Pfam, one TIGRFAM, one whose tree has no alignment) and one alignment without a tree.
    G1 has three copies of PF00001 (the lowest e-value is the last), G2 two copies with rows of different e-values for one gene, G3 lacks
    PF00002, G4 has two copies of TIGR00003 of which the FIRST is best, G5 has an 'unclassified' rank and only one gene.  The paralog
    filter's indexing decides G1 (it looks the later ids up at the wrong positions)."""
    rnd = random.Random(27)
    aa = "ARNDCQEGHILKMFPSTWYV-"
    seq = lambda n: "".join(rnd.choice(aa) for _ in range(n))
    genomes = ["640000001", "640000002", "640000003", "640000004", "640000005"]
    tax = [["Bacteria", "Proteobacteria", "Gammaproteobacteria", "Enterobacterales", "Enterobacteriaceae", "Escherichia", "Escherichia coli"],
           ["Bacteria", "Firmicutes", "Bacilli", "Bacillales", "Bacillaceae", "Bacillus", "Bacillus subtilis"],
           ["Archaea", "Euryarchaeota", "Methanococci", "Methanococcales", "Methanococcaceae", "Methanococcus", "Methanococcus maripaludis"],
           ["Archaea", "Crenarchaeota", "Thermoprotei", "Sulfolobales", "Sulfolobaceae", "Sulfolobus", "unclassified"],
           ["Bacteria", "unclassified", "unclassified", "unclassified", "unclassified", "unclassified", "unclassified Bacteria"]]
    files = {"img_metadata.tsv": "\t".join(METADATA_HEADER) + "\n", "tigrfam2pfam.tsv": ""}
    for g, t in zip(genomes, tax):
        files["img_metadata.tsv"] += "\t".join([g, t[0], "Finished"] + t[1:] + ["1", "5000", "10000", "10", "9000", "Free living", "10000"]) + "\n"
    hits = {g: ([], []) for g in genomes}
    aln = defaultdict(list)

    def add(gene_file, family, genome, gene, evalues, length, tigr=False):
        for e in evalues:
            (hits[genome][1] if tigr else hits[genome][0]).append((tigr_line if tigr else pfam_line)(gene, family, e))
        aln[gene_file].append(">%s|%s extra words\n%s\n" % (genome, gene, seq(length)))

    add("PF00001", "pfam00001", genomes[0], "g1a", ["1e-10"], 12)
    add("PF00001", "pfam00001", genomes[1], "g2a", ["1e-5", "1e-30"], 12)
    add("PF00001", "pfam00001", genomes[0], "g1b", ["1e-20"], 12)
    add("PF00001", "pfam00001", genomes[2], "g3a", ["3e-7"], 12)
    add("PF00001", "pfam00001", genomes[1], "g2b", ["1e-12"], 12)
    add("PF00001", "pfam00001", genomes[0], "g1c", ["1e-40"], 12)
    add("PF00001", "pfam00001", genomes[3], "g4a", ["2e-9"], 12)
    add("PF00002", "pfam00002", genomes[1], "g2c", ["1e-8"], 7)
    add("PF00002", "pfam00002", genomes[0], "g1d", ["1e-3"], 7)
    add("PF00002", "pfam00002", genomes[3], "g4b", ["1e-3"], 7)
    add("TIGR00003", "TIGR00003", genomes[3], "g4c", ["1e-50"], 9, tigr=True)
    add("TIGR00003", "TIGR00003", genomes[4], "g5a", ["1e-2"], 9, tigr=True)
    add("TIGR00003", "TIGR00003", genomes[3], "g4d", ["1e-6"], 9, tigr=True)
    add("TIGR00003", "TIGR00003", genomes[2], "g3b", ["1e-9"], 9, tigr=True)
    add("PF00009", "pfam00009", genomes[0], "g1e", ["1e-9"], 5)                   # an alignment without a gene tree: left out
    for g in genomes:
        files["genomes/%s/%s.pfam.tab.txt" % (g, g)] = "header\n" + "".join(hits[g][0])
        files["genomes/%s/%s.tigrfam.tab.txt" % (g, g)] = "header\n" + "".join(hits[g][1])
    for gene_file, records in aln.items():
        files["alignments/%s.aln.masked.faa" % gene_file] = "".join(records)
    files["alignments/PF00001.other.faa"] = ">x|y\nAAAA\n"                          # another extension: not read
    for gene_file in ("PF00001", "PF00002", "TIGR00003", "PF00777"):
        files["gene_trees/%s.tre" % gene_file] = "(a,b);\n"
    files["gene_trees/notes.txt"] = "not a tree\n"
    return {"name": "five_genomes", "extension": ".aln.masked.faa", "files": files}


def load_class(source, script, name, substitutions, hits, names):
    text = open(os.path.join(source, "scripts", "genometreeworkflow", script)).read()
    m = re.search(r"(?ms)^class %s\(object\):.*?(?=^if __name__)" % name, text)
    if not m:
        raise SystemExit("class %s not found in %s" % (name, script))
    ns = dict(names)
    exec(compile(translate(m.group(0), substitutions, hits), "<%s, translated in memory>" % script, "exec"), ns)
    return ns[name]


def run_concatenate(source, case):
    from checkm.util.img import IMG
    from checkm.util.seqUtils import readFasta, writeFasta
    from checkm.util.taxonomyUtils import appendTaxonomyRanks
    d = tempfile.mkdtemp(prefix="ckm_gtree_golden_")
    for rel, text in case["files"].items():
        p = os.path.join(d, *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    IMG.genomeDir = os.path.join(d, "genomes")

    class ImgStand(object):                                   # the script calls IMG(<two paths of its authors' machine>) and reads IMG.genomeDir / IMG.pfamExtension
        genomeDir, pfamExtension, tigrExtension = IMG.genomeDir, IMG.pfamExtension, IMG.tigrExtension

        def __new__(cls, *_):
            return IMG(os.path.join(d, "img_metadata.tsv"), os.path.join(d, "tigrfam2pfam.tsv"))

    commands = []
    os_stand = types.SimpleNamespace(path=os.path, listdir=os.listdir, system=commands.append)
    Infer = load_class(source, "inferGenomeTree.py", "InferGenomeTree", INFER_SUBSTITUTIONS, INFER_HITS,
                       dict(os=os_stand, defaultdict=defaultdict, IMG=ImgStand, readFasta=readFasta, writeFasta=writeFasta, appendTaxonomyRanks=appendTaxonomyRanks))
    out_aln, out_tree, out_tax = os.path.join(d, "out.faa"), os.path.join(d, "out.tre"), os.path.join(d, "out.tax")
    with contextlib.redirect_stdout(io.StringIO()):
        Infer().run(os.path.join(d, "gene_trees"), os.path.join(d, "alignments"), case["extension"], out_aln, out_tree, out_tax)
    if len(commands) != 1 or not commands[0].startswith("FastTreeMP -nosupport -wag -gamma"):
        raise SystemExit("the script did not reach its FastTree call: %r" % commands)
    return dict(case, alignment=open(out_aln).read(), taxonomy=open(out_tax).read(), order_free=False)


def run_bootstrap(source, seed, alignment_len, num):
    """The columns BootstrapTree.bootstrap draws: the method writes them only through the resampled rows, so the row 'ABC...' of distinct
    symbols spells them out."""
    Boot = load_class(source, "bootstrapTree.py", "BootstrapTree", BOOT_SUBSTITUTIONS, BOOT_HITS, dict(os=os, sys=sys, random=random, open=open))
    symbols = [chr(0x4e00 + k) for k in range(alignment_len)]
    d = tempfile.mkdtemp(prefix="ckm_gtree_boot_")
    random.seed(seed)
    cols = []
    for k in range(num):
        p = os.path.join(d, "b%d.faa" % k)
        Boot().bootstrap({"row": symbols}, p)
        cols.append([ord(ch) - 0x4e00 for ch in open(p).read().split("\n")[1]])
    return {"seed": seed, "alignmentLen": alignment_len, "numBootstraps": num, "cols": cols}


def check_fixture():
    from tests.test_genometree_host import evolved_case, inner, plain_distances, plain_nj
    ids, seqs, truth = evolved_case()
    if inner(plain_nj(plain_distances(seqs, ids, "poisson")), len(ids)) != inner(truth, len(ids)):
        raise SystemExit("the plain neighbour joining does not recover the evolved fixture: choose another seed")


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    if not os.path.isdir(os.path.join(source, "scripts", "genometreeworkflow")):
        raise SystemExit("set CHECKM_SOURCE to the CheckM source tree")
    sys.path.insert(0, source)
    check_fixture()
    out = {"concatenate": [run_concatenate(source, concatenate_case())],
           "bootstrap": [run_bootstrap(source, 1, 17, 3), run_bootstrap(source, 2024, 1, 2), run_bootstrap(source, 7, 64, 1)]}
    path = os.path.join(ROOT, "tests", "golden", "genometree_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
