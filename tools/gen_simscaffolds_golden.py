#!/usr/bin/env python
"""Goldens of the scaffold simulation: the reference's own checkm.util.img.IMG, the class of scripts/genometreeworkflow/markerSetBuilder.py
(sampleGenomeScaffolds*, markerGenesOnScaffolds, buildBinMarkerSet, buildDomainMarkerSet), the worker and writer bodies of
scripts/simulationScaffoldsRandom.py and scripts/simulationScaffoldsByLength.py, and checkm.markerSets, over small hand-made genome
directories and a small tree.  The scripts are Python 2 and do not compile as they stand; their text is loaded in memory after the
substitutions listed below (each counted) and never written to disk.  One substitution is no translation: the contaminant is sampled from
the sorted candidates, because the order of a set of strings depends on the hash seed and current Python refuses to sample from a set.
The scripts' surroundings -- their authors' files, the queues, the output paths under /tmp -- are stand-ins handed to the loaded
functions, not changes of their text; the tree is tests/shim/dendropy's.
Per case and mode: the seed; per replicate the kept ids, the contaminant and its ids, containedMarkerGenes per marker set and both
genomeCheck results as float.hex(); the tuples the worker put on its queue; the writer's two texts.  For the walk: the reference's
buildBinMarkerSet and buildDomainMarkerSet chains, every marker set as sorted lists.  For IMG: the scaffold tables of the genomes.
Runs only where a CheckM source tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_simscaffolds_golden.py              (writes tests/golden/simscaffolds_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_simscaffolds_golden.py --time [--genomes G --scaffolds N --markers M --sets S --replicates R]
                                      (times the reference's markerGenesOnScaffolds + genomeCheck loop on one core over the synthetic
                                       case of tools/simscaffolds_bench.py, writes profiles/r21_simscaffolds_reference_cpu.json)"""
import contextlib
import gzip
import io
import json
import os
import random
import re
import sys
import tempfile
import time
import warnings
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_markerset_golden import all_files, genome, simple, tree as genome_tree, write_tree                        # noqa: E402
from tools.gen_simulation_golden import BUILDER_HITS, BUILDER_SUBSTITUTIONS, Queue, Stand, bin_marker_sets, marker_set, plain, translate      # noqa: E402

SCRIPTS = {"random": "simulationScaffoldsRandom.py", "inv_length": "simulationScaffoldsByLength.py"}
SCRIPT_SUBSTITUTIONS = [("dict.iteritems", r"\.iteritems\(\)", ".items()"),
                        ("xrange", r"\bxrange\(", "range("),
                        ("gzip file of str opened as text", r"(gzip\.open\('[^']*', )'wb'\)", r"\1'wt')"),
                        ("contaminant sampled from the sorted candidates", r"random\.sample\((genomeIdsToTest - set\(\[testGenomeId\]\)), 1\)", r"random.sample(sorted(\1), 1)")]
SCRIPT_HITS = {"dict.iteritems": 1, "xrange": 1, "gzip file of str opened as text": 1, "contaminant sampled from the sorted candidates": 1}


def load_builder(source):
    text = translate(open(os.path.join(source, "scripts", "genometreeworkflow", "markerSetBuilder.py")).read(), BUILDER_SUBSTITUTIONS, BUILDER_HITS)
    ns = {"__name__": "reference_markerSetBuilder"}
    exec(compile(text, "<markerSetBuilder.py, translated in memory>", "exec"), ns)
    return ns["MarkerSetBuilder"]


def load_script(source, mode, read_fasta, open_file, gzip_module):
    """(__seqLens, __workerThread, __writerThread) of the script's SimulationScaffolds as plain functions of (self, ...): the text between
    `def __seqLens` and `def run`, dedented, translated and compiled in memory.  The module's imports (dendropy, its authors' lib package)
    are not run: the names the bodies use are given here."""
    text = open(os.path.join(source, "scripts", SCRIPTS[mode])).read()
    m = re.search(r"(?ms)^    def __seqLens\(.*?(?=^    def run\()", text)
    if not m:
        raise SystemExit("worker and writer bodies not found")
    body = translate(re.sub(r"(?m)^    ", "", m.group(0)), SCRIPT_SUBSTITUTIONS, SCRIPT_HITS)
    from numpy import abs, mean, std
    ns = dict(os=os, sys=sys, random=random, defaultdict=defaultdict, gzip=gzip_module, mean=mean, std=std, abs=abs, readFasta=read_fasta, open=open_file)
    exec(compile(body, "<%s worker and writer, translated in memory>" % SCRIPTS[mode], "exec"), ns)
    return ns["__seqLens"], ns["__workerThread"], ns["__writerThread"]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def scaffolds(prefix, lengths, genes):
    """contigs for tools.gen_markerset_golden.genome: scaffold k is prefix + two digits; genes: scaffold number -> [families] (one gene per entry)"""
    out, n = [], 0
    for k, length in enumerate(lengths):
        mine = []
        for fam in genes.get(k, []):
            n += 1
            mine.append(("%sg%03d" % (prefix, n), 10 * n, 10 * n + 9, [fam] if fam.startswith("pfam") else [], [] if fam.startswith("pfam") else [fam]))
        out.append(("%s%02d" % (prefix, k), length, mine))
    return out


def spread(rng, names, nscaffolds, copies):
    """scaffold number -> families: every family gets one of `copies` copies, each on a scaffold drawn at random"""
    genes = {}
    for m in names:
        for _ in range(rng.choice(copies)):
            genes.setdefault(rng.randrange(nscaffolds), []).append(m)
    return genes


def cases():
    c = []
    # T: twelve scaffolds.  pfam10001 one copy; pfam10002 two copies on ONE scaffold; pfam10005 five copies on five scaffolds; pfam10007 two
    # copies on two scaffolds, and it sits in two co-located sets of UID1; pfam10000 absent from T and present in both contaminants;
    # pfam10009 nowhere; pfam10006's only copy lies on a scaffold the FASTA file lacks ("ghost": it can never be kept); pfam10008 has one
    # gene with a GFF record and one without; t00 carries no marker.  C1 has an eight-field GFF line.  Two sets of the chain share a
    # lineageStr, and the refined chain lacks it.
    T = genome(scaffolds("t", [900, 700, 600, 500, 400, 350, 300, 250, 200, 150, 100, 80],
                         {0: ["pfam19999"], 1: ["pfam10001"], 2: ["pfam10002", "pfam10002"], 3: ["pfam10005"], 4: ["pfam10005"], 5: ["pfam10005"], 6: ["pfam10005"],
                          7: ["pfam10005", "pfam10007"], 8: ["TIGR10001"], 9: ["pfam10007"], 10: ["pfam10008"], 11: ["pfam19999"]}),
               pfam_extra=[("tghost", "pfam10006"), ("tnogff", "pfam10008")])
    T[".gff"] += "ghost\timg\tCDS\t5\t50\t.\t+\t0\tID=tghost;locus_tag=L_tghost\n"      # the last record: geneDistTable looks up a contig's length when it leaves it
    C1 = genome(scaffolds("c", [500, 400, 300, 200, 100, 50], {0: ["pfam10000"], 1: ["pfam10001"], 2: ["pfam10007"], 4: ["pfam10005", "pfam10005"]}),
                gff_extra=["c00\timg\tCRISPR\t5\t7\t.\t+\t0\n"])
    C2 = genome(scaffolds("d", [450, 350, 250, 150, 90], {0: ["pfam10000", "TIGR10001"], 1: ["pfam10000"], 3: ["pfam10002"]}))
    chain = [marker_set("UID1", "k__Bacteria;p__X", 40, [["pfam10001", "pfam10002"], ["pfam10005", "pfam10000", "pfam10007"], ["pfam10007", "pfam10006", "pfam10009"], ["TIGR10001"],
                                                         ["pfam10008"]]),
             marker_set("UID2", "k__Bacteria", 200, [["pfam10001", "pfam10005", "pfam10007"], ["pfam10000"]]),
             marker_set("UID3", "k__Bacteria", 900, [["pfam10005"], ["pfam10002", "pfam10009", "TIGR10001"]])]
    refined = [marker_set("UID1", "k__Bacteria;p__X", 40, [["pfam10001", "pfam10002"], ["pfam10005", "pfam10007"], ["pfam10008"]])]
    c.append(dict(name="copies", seed=7, genomes={"T": T, "C1": C1, "C2": C2}, genomeId="T", candidates=["T", "C1", "C2"], taxonomy=["Bacteria", "X", "Y"], numReplicates=2,
                  contigLens=[5000, 20000], percentComps=[0.5, 1.0], percentConts=[0.0, 0.2], chain=chain, refined=refined))
    # co-located sets of three and of seven markers, twelve of them: the quotients do not sum exactly, and the order of the sum shows
    rng = random.Random(13)
    sizes = [3, 7] * 6
    names = ["pfam2%04d" % k for k in range(sum(sizes))]
    tg, cg, dg = spread(rng, names, 14, [0, 1, 1, 1, 1, 2, 3]), spread(rng, names, 8, [0, 0, 1, 1]), spread(rng, names, 6, [0, 0, 0, 1, 2])
    sets, at = [], 0
    for n in sizes:
        sets.append(names[at:at + n]); at += n
    shuffled = names[:]
    rng.shuffle(shuffled)
    other = [shuffled[k:k + 3] for k in range(0, 60, 3)]
    chain = [marker_set("UID10", "k__Bacteria;p__Thirds", 55, sets), marker_set("UID11", "k__Bacteria", 3000, other)]
    refined = [marker_set("UID10", "k__Bacteria;p__Thirds", 55, sets[:9]), marker_set("UID11", "k__Bacteria", 3000, other[:10] + [names[53:60]])]
    lens = lambda n, seed: [random.Random(seed).randrange(40, 400) for _ in range(n)]
    c.append(dict(name="thirds_and_sevenths", seed=14, genomes={"T2": genome(scaffolds("u", lens(14, 1), tg)), "C3": genome(scaffolds("v", lens(8, 2), cg)),
                                                                   "C4": genome(scaffolds("w", lens(6, 3), dg))},
                  genomeId="T2", candidates=["C3", "C4", "T2"], taxonomy=["Bacteria", "Thirds"], numReplicates=1, contigLens=[5000], percentComps=[0.5, 1.0], percentConts=[0.0, 0.2],
                  chain=chain, refined=refined))
    return c


def walk_case():
    """A tree of seven leaves.  IMG_W7 is no leaf: the derep list holds it as a duplicate of IMG_W3.  UID5 keeps one genome once W1 is
    removed; UID4 and UID6 have no taxonomy and lie between named nodes; with root_named False the root has none either."""
    newick = "((((IMG_W1,IMG_W2)UID5|c__C|90,(IMG_W3,IMG_W4)UID6||80)UID4||70,IMG_W5)UID3|p__P|60,(IMG_W6,IMG_W8)UID7|p__Q|50)UID2|k__Bacteria|100;\n"
    fams = lambda *extra: [("pfam30001", 1000), ("pfam30002", 2000), ("pfam30003", 9000)] + list(extra)
    genomes = {"W1": simple(fams(("pfam30005", 30000))), "W2": simple(fams(("pfam30005", 30000))), "W3": simple(fams(("pfam30006", 40000))), "W4": simple(fams(("pfam30006", 40500))),
               "W5": simple([("pfam30001", 1000), ("pfam30002", 2000), ("pfam30006", 40000)]), "W6": simple(fams(("pfam30002", 60000), ("pfam30004", 50000))),
               "W7": simple(fams(("pfam30006", 43000), ("TIGR30001", 70000))), "W8": simple(fams(("pfam30004", 50000), ("TIGR30001", 70000)))}
    taxonomy = {"UID2": "k__Bacteria", "UID3": "k__Bacteria;p__P", "UID4": "", "UID5": "k__Bacteria;p__P;c__C", "UID6": "", "UID7": "k__Bacteria;p__Q"}

    def metadata(root_named):
        text = "UID\t# genomes\tTaxonomy\tBootstrap\tGC mean\tGC std\tGenome size mean\tGenome size std\tGene count mean\tGene count std\tMarker set\n"
        for k, (uid, tax) in enumerate(sorted(taxonomy.items())):
            if uid == "UID2" and not root_named:
                tax = ""
            text += "%s\t%d\t%s\t%s\t50.0\t1.0\t3000000\t100000\t3000\t100\t[set(['pfam30001'])]\n" % (uid, 2 + k, tax, "NA" if uid == "UID6" else "90.0")
        return text

    removal = {"UID2": [[], []], "UID3": [["pfam30003"], []], "UID4": [[], []], "UID5": [["pfam30003"], ["pfam30002"]], "UID6": [["pfam30006"], []], "UID7": [[], ["pfam30002"]]}
    py2 = lambda genes: "set([%s])" % ", ".join("'%s'" % g for g in genes)
    files, same_as = genome_tree(genomes)
    return dict(name="walk", newick=newick, files=files, same_as=same_as, redundant="pfam30006\tTIGR30001\n", derep="IMG_W1\nIMG_W3 IMG_W7\nIMG_W4\n",
                metadata_named=metadata(True), metadata_root_unnamed=metadata(False),
                missing_duplicate="".join("%s\t%s\t%s\n" % (uid, py2(m), py2(d)) for uid, (m, d) in sorted(removal.items())),
                ubiquity=0.7, single=0.7, starts=["W1", "W3", "W5", "W6"])


def sets_of(binMarkerSets):
    return [dict(lineageStr=ms.lineageStr, numGenomes=ms.numGenomes, UID=ms.UID, sets=sorted(sorted(s) for s in ms.markerSet)) for ms in binMarkerSets.markerSetIter()]


def reference_img(IMG, d):
    IMG.genomeDir = d + os.sep
    return IMG(os.path.join(d, "img_metadata.tsv"), os.path.join(d, "tigrfam2pfam.tsv"))


def run_walk(Builder, IMG, c):
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import dendropy
    d = write_tree(tempfile.mkdtemp(prefix="ckm_simscaf_walk_"), c)
    tree = dendropy.Tree.get_from_string(c["newick"], "newick", preserve_underscores=True)
    out = []
    for root_named in (True, False):
        b = object.__new__(Builder)                     # the reference's __init__ and its readers open files of its authors' machine
        b.img, b.cachedGeneCountTable = reference_img(IMG, d), None
        b.duplicateSeqs = {f[0]: f[1:] for f in (line.split() for line in c["derep"].splitlines()) if len(f) > 1}
        b.uniqueIdToLineageStatistics = {}
        for line in c["metadata_named" if root_named else "metadata_root_unnamed"].splitlines()[1:]:
            f = line.split("\t")
            b.uniqueIdToLineageStatistics[f[0]] = {"taxonomy": f[2]}
        b.lineageSpecificGenesToRemove = {}
        for line in c["missing_duplicate"].splitlines():
            f = line.split("\t")
            b.lineageSpecificGenesToRemove[f[0]] = eval(f[1]).union(eval(f[2]))
        for g in c["starts"]:
            node = tree.find_node_with_taxon_label("IMG_" + g).parent_node
            for bMarkerSet in (True, False):
                for domain in (False, True):
                    build = b.buildDomainMarkerSet if domain else b.buildBinMarkerSet
                    with contextlib.redirect_stdout(io.StringIO()):
                        chain, refined = build(tree, node, c["ubiquity"], c["single"], bMarkerSet=bMarkerSet, genomeIdsToRemove=[g])
                    out.append(dict(root_named=root_named, genomeId=g, bMarkerSet=bMarkerSet, domain=domain, binId=chain.binId, chain=sets_of(chain), refined=sets_of(refined)))
    return dict(c, chains=out)


def run_img(IMG, d, ids):
    img = reference_img(IMG, d)
    out = {}
    for g in ids:
        table = img._genomeIdToClusterScaffold(g)
        out[g] = dict(cluster_scaffold={f: sorted(v) for f, v in sorted(table.items())}, seq_ids=list(img._genomeSeqLens(g).keys()))
    if "T" in out:
        out["T"]["gene_scaffold"] = img.geneIdToScaffoldId("T")      # (C1's eight-field line makes the reference's geneIdToScaffoldId fail)
    metadata = {"A": {"status": "Finished"}, "B": {"status": "Draft"}, "C": {"status": "Finished"}}
    out["filter"] = dict(metadata=metadata, genomeIds=["A", "B", "C"], field="status", value="Finished", kept=sorted(img.filterGenomeIds(["A", "B", "C"], metadata, "status", "Finished")))
    return out


def run_case(Builder, IMG, MarkerSet, BinMarkerSets, source, c):
    from checkm.util.seqUtils import readFasta
    files, same_as = genome_tree(c["genomes"])
    c = dict({k: v for k, v in c.items() if k != "genomes"}, files=files, same_as=same_as, redundant="")
    d = write_tree(tempfile.mkdtemp(prefix="ckm_simscaf_golden_"), c)
    ids = sorted(set(rel.split("/")[0] for rel in all_files(c)))
    chain, refined = bin_marker_sets(MarkerSet, BinMarkerSets, c["genomeId"], c["chain"]), bin_marker_sets(MarkerSet, BinMarkerSets, c["genomeId"], c["refined"])
    marker_sets = list(chain.markerSetIter()) + list(refined.markerSetIter())
    runs = {}
    for mode in sorted(SCRIPTS):
        img = reference_img(IMG, d)
        img.precomputeGenomeFamilyScaffolds(ids)
        b = object.__new__(Builder)
        b.img = img
        b.buildBinMarkerSet = lambda *a, **k: (chain, refined)
        sim = Stand(markerSetBuilder=b, img=img, contigLens=c["contigLens"], percentComps=c["percentComps"], percentConts=c["percentConts"])
        redirect = lambda path: os.path.join(d, mode + "." + os.path.basename(path))
        seq_lens, worker, writer = load_script(source, mode, readFasta, lambda path, mode_: open(redirect(path), mode_), Stand(open=lambda path, mode_: gzip.open(redirect(path), mode_)))
        setattr(sim, "__seqLens", lambda seqs: seq_lens(sim, seqs))
        tree = Stand(find_node_with_taxon_label=lambda label: Stand(parent_node=None))
        out = Queue()
        random.seed(c["seed"]); np.random.seed(c["seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            worker(sim, tree, {c["genomeId"]: dict(taxonomy=c["taxonomy"])}, set(c["candidates"]), 0.97, 0.97, c["numReplicates"], Queue([c["genomeId"], None]), out)
        tuples = list(out.items)
        recorded = plain(tuples)                          # as they leave the worker: the writer's lookups add keys to the defaultdicts it is handed
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            writer(sim, 1, Queue(tuples + [(None,) * 18]))
        texts = sorted(os.listdir(d))
        summary = open([os.path.join(d, f) for f in texts if f.startswith(mode + ".") and f.endswith(".tsv")][0]).read()
        replicates = gzip.open([os.path.join(d, f) for f in texts if f.startswith(mode + ".") and f.endswith(".tsv.gz")][0], "rt").read()
        # the same draws again with the reference's samplers in the script's order, each scored the way the worker scores it
        random.seed(c["seed"]); np.random.seed(c["seed"])
        lens_of = lambda g: seq_lens(sim, readFasta(os.path.join(d, g, g + ".fna")))
        testSeqLens, genomeSize = lens_of(c["genomeId"])
        draws = []
        for contigLen in c["contigLens"]:
            for percentComp in c["percentComps"]:
                for percentCont in c["percentConts"]:
                    for _ in range(c["numReplicates"]):
                        if mode == "random":
                            retained, trueComp = b.sampleGenomeScaffoldsWithoutReplacement(percentComp, testSeqLens, genomeSize)
                        else:
                            removed, per = b.sampleGenomeScaffoldsInvLength(1.0 - percentComp, testSeqLens, genomeSize)
                            trueComp, retained = 100.0 - per, [s for s in testSeqLens if s not in removed]
                        cont = random.sample(sorted(set(c["candidates"]) - set([c["genomeId"]])), 1)[0]
                        contSeqLens, contSize = lens_of(cont)
                        if mode == "random":
                            keep, per = b.sampleGenomeScaffoldsWithoutReplacement(1 - percentCont, contSeqLens, contSize)
                            sampled, trueCont = set(contSeqLens.keys()).difference(keep), 100.0 - per
                        else:
                            sampled, trueCont = b.sampleGenomeScaffoldsInvLength(percentCont, contSeqLens, contSize)
                        draws.append(dict(contigLen=contigLen, percentComp=percentComp, percentCont=percentCont, retained=[str(s) for s in retained], contGenomeId=cont,
                                          contSampled=sorted(str(s) for s in sampled), trueComp=float(trueComp), trueCont=float(trueCont)))
        assert [x["trueComp"] for x in draws] == [v for t in tuples for v in t[16]] and [x["trueCont"] for x in draws] == [v for t in tuples for v in t[17]]
        for x in draws:
            x["contained"], x["checks"] = [], []
            for ms in marker_sets:
                contained = defaultdict(list)
                b.markerGenesOnScaffolds(ms.getMarkerGenes(), c["genomeId"], x["retained"], contained)
                b.markerGenesOnScaffolds(ms.getMarkerGenes(), x["contGenomeId"], x["contSampled"], contained)
                x["contained"].append({m: sorted(v) for m, v in sorted(contained.items())})
                x["checks"].append([v.hex() for v in ms.genomeCheck(contained, bIndividualMarkers=True) + ms.genomeCheck(contained, bIndividualMarkers=False)])
        # the worker's deltas are these checks minus the true values, replicate by replicate
        k = 0
        for t in tuples:
            seen = defaultdict(int)
            for _ in range(c["numReplicates"]):
                x = draws[k]; k += 1
                for ms, row in zip(list(chain.markerSetIter()), x["checks"]):
                    assert t[8][ms.lineageStr][seen[ms.lineageStr]] == float.fromhex(row[0]) - x["trueComp"] and t[11][ms.lineageStr][seen[ms.lineageStr]] == float.fromhex(row[3]) - x["trueCont"]
                    seen[ms.lineageStr] += 1
        runs[mode] = dict(draws=draws, tuples=recorded, summary=summary, replicates=replicates)
    c["img"] = run_img(IMG, d, ids)
    return dict(c, runs=runs)


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    os.environ["CHECKM_DATA_PATH"] = tempfile.mkdtemp(prefix="ckm_simscaf_data_")      # the reference's import otherwise creates ~/.checkm
    sys.path.insert(0, source)
    from checkm.markerSets import BinMarkerSets, MarkerSet
    from checkm.util.img import IMG
    Builder = load_builder(source)
    if "--time" in sys.argv:
        return time_reference(Builder, MarkerSet)
    head = dict(generator="tools/gen_simscaffolds_golden.py: checkm.util.img.IMG, the class of scripts/genometreeworkflow/markerSetBuilder.py, the worker and writer bodies of "
                          "scripts/simulationScaffoldsRandom.py and scripts/simulationScaffoldsByLength.py and checkm.markerSets of the reference, the scripts loaded in memory after the "
                          "substitutions the tool lists",
                substitutions=dict(markerSetBuilder=[s[0] for s in BUILDER_SUBSTITUTIONS], scripts=[s[0] for s in SCRIPT_SUBSTITUTIONS]))
    done = [run_case(Builder, IMG, MarkerSet, BinMarkerSets, source, c) for c in cases()]
    walk = run_walk(Builder, IMG, walk_case())
    path = os.path.join(ROOT, "tests", "golden", "simscaffolds_cases.json")
    lines = ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in done)          # a case per line
    open(path, "w").write(json.dumps(head, sort_keys=True)[:-1] + ', "walk": ' + json.dumps(walk, sort_keys=True, separators=(",", ":")) + ',\n"cases": [\n' + lines + "\n]}\n")
    for c in done:
        for mode, r in sorted(c["runs"].items()):
            print(c["name"], mode, len(r["draws"]), "draws", len(r["tuples"]), "tuples", len(r["summary"]), len(r["replicates"]), "bytes of text")
    print(len(walk["chains"]), "chains of the walk")
    print(os.path.getsize(path), "bytes")


def time_reference(Builder, MarkerSet):
    from tools.simscaffolds_bench import synth_case, synth_draws
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    G, N, M, S, R = arg("--genomes", 200), arg("--scaffolds", 300), arg("--markers", 1500), arg("--sets", 20), arg("--replicates", 20)
    scaffolds_of, seq_lens, chain = synth_case(G, N, M, S, seed=21)
    sets = [MarkerSet(ms.UID, ms.lineageStr, ms.numGenomes, [set(s) for s in ms.markerSet]) for ms in chain]
    b = object.__new__(Builder)
    b.img = Stand(cachedGenomeFamilyScaffolds=scaffolds_of)
    test = sorted(scaffolds_of)[0]
    draws = synth_draws(seq_lens, test, R, seed=21)
    t0 = time.perf_counter()
    for retained, cont, sampled in draws:
        for ms in sets:
            contained = defaultdict(list)
            b.markerGenesOnScaffolds(ms.getMarkerGenes(), test, retained, contained)
            b.markerGenesOnScaffolds(ms.getMarkerGenes(), cont, sampled, contained)
            ms.genomeCheck(contained, bIndividualMarkers=True)
            ms.genomeCheck(contained, bIndividualMarkers=False)
    wall = time.perf_counter() - t0
    out = dict(what="reference markerGenesOnScaffolds (test genome and contaminant) + both genomeCheck modes (translated in memory), one core, the synthetic case of "
                    "tools/simscaffolds_bench.py, one test genome", genomes=G, scaffolds=N, markers=M, sets=S, replicates=R, checks=R * S, seconds=wall,
               seconds_per_replicate_set_check=wall / (R * S), replicate_set_checks_per_second=R * S / wall)
    open(os.path.join(ROOT, "profiles", "r21_simscaffolds_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
