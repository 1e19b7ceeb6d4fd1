#!/usr/bin/env python
"""Goldens of the marker-set selection: the class of scripts/simInferBestMarkerSet.py (its __selectMarkerSet and __writerThread) and the
class of scripts/createSelectedMarkerSetMapping.py of the reference, with the reference's own checkm.util.img.IMG, the class of
scripts/genometreeworkflow/markerSetBuilder.py and checkm.markerSets, over a small synthetic tree and genome directory.  The scripts are
Python 2 and do not compile as they stand; their class text is loaded in memory after the substitutions listed below (each counted) and
never written to disk.  One substitution is no translation: the test genomes are sampled from the SORTED child lineage, because the order
of a set of strings depends on the hash seed and current Python refuses to sample from a set.  The scripts' surroundings -- their authors'
files, the queues, the output paths -- are stand-ins handed to the loaded classes, not changes of their text; the tree is
tests/shim/dendropy's; simContigLen is the attribute the script's __init__ sets, here 50 so that the genomes stay small.
Per internal node with a parent: the seed both generators got, and the tuple the script put on its queue (floats as float.hex()).  Then
the writer's table and the mapping script's file.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_selection_golden.py              (writes tests/golden/selection_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_selection_golden.py --time [--genomes G --mb N --markers M --sets S]
                                      (times the reference's replicate loop on one core over the synthetic node of
                                       tools/selection_bench.py, writes profiles/r22_selection_reference_cpu.json)"""
import contextlib
import io
import json
import os
import random
import re
import sys
import tempfile
import time
import zlib
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_markerset_golden import genome, tree as genome_tree, write_tree                                          # noqa: E402
from tools.gen_simscaffolds_golden import load_builder, reference_img                                                    # noqa: E402
from tools.gen_simulation_golden import BUILDER_SUBSTITUTIONS, Queue, Stand, translate                                   # noqa: E402

INFER_SUBSTITUTIONS = [("xrange", r"\bxrange\(", "range("),
                       ("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)"),
                       ("test genomes sampled from the sorted child", r"random\.sample\(orderedLeaves\[0\], ", "random.sample(sorted(orderedLeaves[0]), ")]
INFER_HITS = {"xrange": 1, "print statements": 8, "test genomes sampled from the sorted child": 1}
MAPPING_SUBSTITUTIONS = [("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)")]
MAPPING_HITS = {"print statements": 1}
CONTIG_LEN = 50


def load_class(source, script, name, substitutions, hits, names):
    """The class `name` of a script: its text up to the script's __main__ part, translated and compiled in memory.  The module's imports
    (dendropy's Taxon, its authors' lib package) are not run: the names the class uses are given here."""
    text = open(os.path.join(source, "scripts", script)).read()
    m = re.search(r"(?ms)^class %s\(object\):.*?(?=^if __name__)" % name, text)
    if not m:
        raise SystemExit("class %s not found in %s" % (name, script))
    ns = dict(names)
    exec(compile(translate(m.group(0), substitutions, hits), "<%s, translated in memory>" % script, "exec"), ns)
    return ns[name]


def node_seed(seed, uid):
    return ((seed & 0xffffffff) << 32) | zlib.crc32(uid.encode())


# ---- the case ---------------------------------------------------------------------------------------------------------------------------------
def selection_case():
    """Three clades below the root.  UID3: children UID5 (A1..A5) and UID6 (B1..B5): eligible (equal sizes: the first child), the A genomes are tested.  UID7: children
    UID8 (C1..C4 and C5, which is no leaf: the derep list holds it as a duplicate of IMG_C4) and UID9 (D1..D5): eligible through the
    duplicate.  UID10: children UID11 (E1..E4) and UID12 (F1..F5): its smallest child has 4 genomes, 'NA'.  Every node above leaves alone
    has children of one genome: 'NA'.  UID6 and UID9 have no taxonomy.  Families: universal ones in every genome, clade families in one
    clade, some with a second copy, some missing (enough of them that no draw leaves a set without any: the script exits on a completeness of 0.0); genes lie anywhere in the genome, in its partial tail, and a few beyond its end.  Only the
    tested genomes (A, C) differ from each other throughout; the others repeat a few files, which the JSON stores once."""
    rng = random.Random(22)
    clades = {"A": 5, "B": 5, "C": 5, "D": 5}
    universal = ["pfam5%04d" % k for k in range(28)] + ["TIGR5%04d" % k for k in range(2)]
    of_clade = {"AB": ["pfam6%04d" % k for k in range(6)], "CD": ["pfam7%04d" % k for k in range(6)]}
    genomes = {}
    for clade, n in clades.items():
        for k in range(1, n + 1):
            if clade in "BD" and k > 2:                               # B3..B5 and D3..D5 repeat B1, B2, D1, D2: they only count in the thresholds
                genomes["%s%d" % (clade, k)] = genomes["%s%d" % (clade, 1 + k % 2)]
                continue
            length = rng.randrange(1000, 2000)
            fams = []
            for f in universal + [f for pair, fs in of_clade.items() if clade in pair for f in fs]:
                copies = rng.choice([0] + [1] * 22 + [2])
                fams.extend(f for _ in range(copies))
            genes = []
            for j, f in enumerate(fams):
                start = rng.randrange(1, length + 80) if rng.random() < 0.9 else length - length % CONTIG_LEN + rng.randrange(0, CONTIG_LEN)
                genes.append(("%s%dg%02d" % (clade.lower(), k, j), start, start + 40, [f] if f.startswith("pfam") else [], [] if f.startswith("pfam") else [f]))
            genomes["%s%d" % (clade, k)] = genome([("c1", length, genes)])
    for k in range(1, 10):                                            # the E and F genomes repeat D1 and D2
        genomes[("E%d" % k) if k < 5 else ("F%d" % (k - 4))] = genomes["D%d" % (1 + k % 2)]
    leaves = lambda clade, n: ",".join("IMG_%s%d" % (clade, k) for k in range(1, n + 1))
    newick = ("((({A})UID5|c__A|90,({B})UID6||80)UID3|p__P|70,(({C})UID8|c__C|60,({D})UID9||50)UID7|p__Q|60,(({E})UID11|c__E|60,({F})UID12|c__F|50)UID10|p__R|60)"
              "UID2|k__Bacteria|100;\n").format(A=leaves("A", 5), B=leaves("B", 5), C=leaves("C", 4), D=leaves("D", 5), E=leaves("E", 4), F=leaves("F", 5))
    taxonomy = {"UID2": "k__Bacteria", "UID3": "k__Bacteria;p__P", "UID5": "k__Bacteria;p__P;c__A", "UID6": "", "UID7": "k__Bacteria;p__Q", "UID8": "k__Bacteria;p__Q;c__C",
                "UID9": "", "UID10": "k__Bacteria;p__R", "UID11": "k__Bacteria;p__R;c__E", "UID12": "k__Bacteria;p__R;c__F"}
    metadata = "UID\t# genomes\tTaxonomy\tBootstrap\tGC mean\tGC std\tGenome size mean\tGenome size std\tGene count mean\tGene count std\tMarker set\n"
    for k, (uid, tax) in enumerate(sorted(taxonomy.items())):
        metadata += "%s\t%d\t%s\t90.0\t50.0\t1.0\t3000000\t100000\t3000\t100\t[set(['pfam50001'])]\n" % (uid, 2 + k, tax)
    files, same_as = genome_tree(genomes)
    return dict(name="selection", newick=newick, files=files, same_as=same_as, redundant="", derep="IMG_A1\nIMG_C4 IMG_C5\n", metadata=metadata,
                missing_duplicate="".join("%s\tset([])\tset([])\n" % uid for uid in sorted(taxonomy)), ubiquity=0.8, single=0.8, simContigLen=CONTIG_LEN, seed=22)


def reference_builder(Builder, IMG, d, c):
    b = object.__new__(Builder)                     # the reference's __init__ and its readers open files of its authors' machine
    b.img, b.cachedGeneCountTable = reference_img(IMG, d), None
    b.duplicateSeqs = {f[0]: f[1:] for f in (line.split() for line in c["derep"].splitlines()) if len(f) > 1}
    b.uniqueIdToLineageStatistics = {line.split("\t")[0]: {"taxonomy": line.split("\t")[2]} for line in c["metadata"].splitlines()[1:]}
    b.lineageSpecificGenesToRemove = {line.split("\t")[0]: set() for line in c["missing_duplicate"].splitlines()}
    return b


def run_case(source, Builder, IMG, c):
    from checkm.util.seqUtils import readFastaBases
    from numpy import abs, array, mean, percentile, std
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import dendropy
    d = write_tree(tempfile.mkdtemp(prefix="ckm_selection_golden_"), c)
    tree = dendropy.Tree.get_from_string(c["newick"], "newick", preserve_underscores=True)
    redirect = lambda path: os.path.join(d, os.path.basename(path))
    stand_open = lambda path, mode="r": open(redirect(path), mode)
    Simulation = load_class(source, "simInferBestMarkerSet.py", "Simulation", INFER_SUBSTITUTIONS, INFER_HITS,
                            dict(os=os, sys=sys, random=random, defaultdict=defaultdict, mean=mean, std=std, abs=abs, percentile=percentile, array=array,
                                 readFastaBases=readFastaBases, open=stand_open, mp=None, dendropy=dendropy))
    sim = object.__new__(Simulation)                # its __init__ makes the builder and IMG of its authors' machine
    sim.markerSetBuilder = reference_builder(Builder, IMG, d, c)
    sim.img = sim.markerSetBuilder.img
    sim.img.genomeDir = d + os.sep
    sim.simContigLen = c["simContigLen"]
    nodes, tuples = [], []
    for node in tree.internal_nodes():
        if node.parent_node is None:
            continue
        uid = node.label.split("|")[0]
        seed = node_seed(c["seed"], uid)
        random.seed(seed); np.random.seed(seed & 0xffffffff)
        out = Queue()
        with contextlib.redirect_stdout(io.StringIO()):
            getattr(sim, "_Simulation__selectMarkerSet")(tree, node, None, c["ubiquity"], c["single"], out)
        t = out.items[0]
        tuples.append(t)
        nodes.append(dict(label=node.label, seed=seed, tuple=["NA" if isinstance(t[0], str) else t[0].label] + [x if isinstance(x, (str, int)) or x is None else float(x).hex() for x in t[1:]]))
    with contextlib.redirect_stdout(io.StringIO()):
        getattr(sim, "_Simulation__writerThread")(len(tuples), Queue(tuples + [(None,) * 6]))
    table = open(os.path.join(d, "simInferBestMarkerSet.tsv")).read()
    Mapping = load_class(source, "createSelectedMarkerSetMapping.py", "CreateSelectedMarkerSetMapping", MAPPING_SUBSTITUTIONS, MAPPING_HITS,
                         dict(os=os, sys=sys, open=stand_open, dendropy=Stand(Tree=Stand(get_from_path=lambda *a, **k: tree))))
    with contextlib.redirect_stdout(io.StringIO()):
        Mapping().run()
    selected = open(os.path.join(d, "selected_marker_sets.tsv")).read()
    # the mapping of a table in which one node's set is 'NA' and one carries a lineage string: the walk up, and the split at '|'
    edited = table.splitlines(True)
    edited = [edited[0]] + [line.replace("\tUID", "\tNA | was UID", 1) if k == 0 else line for k, line in enumerate(edited[1:])] + ["UID12|c__F|50\tUID10 | p__R\t1.00\t1.00\t1.00\t1.00\n"]
    open(os.path.join(d, "simInferBestMarkerSet.tsv"), "w").write("".join(edited))
    with contextlib.redirect_stdout(io.StringIO()):
        Mapping().run()
    return dict(c, nodes=nodes, table=table, selected=selected, edited_table="".join(edited), edited_selected=open(os.path.join(d, "selected_marker_sets.tsv")).read())


def time_reference(source, Builder):
    from numpy import abs, array, mean, percentile, std
    from checkm.markerSets import BinMarkerSets, MarkerSet
    from tools.selection_bench import synth_node
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    G, mb, M, S = max(arg("--genomes", 5), 5), arg("--mb", 5), arg("--markers", 1500), arg("--sets", 6)
    sets, positions, sizes = synth_node(G, mb, M, S, seed=22)
    chain = BinMarkerSets("node", BinMarkerSets.TREE_MARKER_SET)
    for ms in sets:
        chain.addMarkerSet(MarkerSet(ms.UID, ms.lineageStr, ms.numGenomes, [set(s) for s in ms.markerSet]))
    ids = ["G%03d" % g for g in range(G)]
    size_of = {os.path.join("dir", g, g + ".fna"): n for g, n in zip(ids, sizes)}
    Simulation = load_class(source, "simInferBestMarkerSet.py", "Simulation", INFER_SUBSTITUTIONS, INFER_HITS,
                            dict(os=os, sys=sys, random=random, defaultdict=defaultdict, mean=mean, std=std, abs=abs, percentile=percentile, array=array,
                                 readFastaBases=lambda path: size_of[path], mp=None, dendropy=None))
    sim = object.__new__(Simulation)
    b = object.__new__(Builder)
    b.duplicateSeqs = {}
    b.buildBinMarkerSet = lambda *a, **k: (chain, None)
    sim.markerSetBuilder = b
    sim.img = Stand(genomeDir="dir", geneDistTable=lambda genomeIds, markerGenes, spacingBetweenContigs=0: {g: positions[ids.index(g)] for g in genomeIds})
    sim.simContigLen = 10000
    child = lambda names: Stand(leaf_nodes=lambda: [Stand(taxon=Stand(label="IMG_" + g)) for g in names])
    node = Stand(label="UID1|x|1", child_nodes=lambda: [child(ids), child(["other%d" % k for k in range(G + 1)])])      # the smaller child: the test genomes
    random.seed(22); np.random.seed(22)
    out = Queue()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        getattr(sim, "_Simulation__selectMarkerSet")(None, node, None, 0.97, 0.97, out)
    wall = time.perf_counter() - t0
    draws = len(ids) * 100
    res = dict(what="reference __selectMarkerSet of scripts/simInferBestMarkerSet.py (translated in memory; its replicate loop: random.uniform, sampleGenome, containedMarkerGenes and "
                    "genomeCheck per set), one core, the synthetic node of tools/selection_bench.py", genomes=len(ids), mb=mb, markers=M, sets=S, replicates_per_genome=100,
               draws=draws, seconds=wall, draws_per_second=draws / wall, seconds_per_draw=wall / draws)
    open(os.path.join(ROOT, "profiles", "r22_selection_reference_cpu.json"), "w").write(json.dumps(res) + "\n")
    print(json.dumps(res))


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    os.environ["CHECKM_DATA_PATH"] = tempfile.mkdtemp(prefix="ckm_selection_data_")      # the reference's import otherwise creates ~/.checkm
    sys.path.insert(0, source)
    from checkm.util.img import IMG
    Builder = load_builder(source)
    if "--time" in sys.argv:
        return time_reference(source, Builder)
    head = dict(generator="tools/gen_selection_golden.py: the classes of scripts/simInferBestMarkerSet.py and scripts/createSelectedMarkerSetMapping.py, checkm.util.img.IMG, the class of "
                          "scripts/genometreeworkflow/markerSetBuilder.py and checkm.markerSets of the reference, the scripts loaded in memory after the substitutions the tool lists",
                substitutions=dict(markerSetBuilder=[s[0] for s in BUILDER_SUBSTITUTIONS], simInferBestMarkerSet=[s[0] for s in INFER_SUBSTITUTIONS],
                                   createSelectedMarkerSetMapping=[s[0] for s in MAPPING_SUBSTITUTIONS]))
    done = run_case(source, Builder, IMG, selection_case())
    path = os.path.join(ROOT, "tests", "golden", "selection_cases.json")
    whole = dict(head, **done)
    files = whole.pop("files")                                        # a key per line, a file per line
    lines = [json.dumps(k) + ":" + json.dumps(v, sort_keys=True, separators=(",", ":")) for k, v in sorted(whole.items())]
    lines.append('"files":{\n' + ",\n".join(json.dumps(k) + ":" + json.dumps(v) for k, v in sorted(files.items())) + "\n}")
    open(path, "w").write("{\n" + ",\n".join(lines) + "\n}\n")
    for n in done["nodes"]:
        print(n["label"], n["tuple"][:2])
    print(done["table"])
    print(done["selected"])
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
