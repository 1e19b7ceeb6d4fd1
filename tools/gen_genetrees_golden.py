#!/usr/bin/env python
"""Goldens of GeneTrees' two tests: the classes of scripts/genometreeworkflow/paralogTest.py and consistencyTest.py of the reference over
small synthetic forests.  The scripts are Python 2 and do not compile as they stand; their class text is loaded in memory after the
substitutions listed below (each counted) and never written to disk.  The scripts' surroundings are stand-ins handed to the loaded
classes, not changes of their text:
  IMG         a callable that ignores the paths of the authors' machine and gives the case's metadata;
  os, open    the real ones, but a path under /srv (the TIGRFAM INFO directory, Pfam-A.clans.tsv) is answered from the case's own
              files, listdir is sorted, and system('cp a b') copies and records;
  RerootTree  GenomeTree.reroot (DESIGN §27's rule) with the outgroup rerootTree.py:59-76 collects, put back into the tree object so
              that the leaf objects the script holds stay its leaves;
  dendropy    tests/shim/dendropy.py (not edited) with what the two scripts need on top, defined here.  What it pins:
                mrca(taxon_labels=)   the deepest node whose subtree holds every named leaf (below a chain of single-child nodes: the
                                      lowest of the chain);
                distance_from_root()  the node's own edge length first, then every ancestor's on the way up, the root's own last when
                                      it has one (DendroPy's loop): ((leaf + parent) + grandparent) + ...;
                edge_length, parent_node: the shim's attributes.
What the prints and the files do not show is observed through the stand-ins: the genomes with paralogs are the keys of the defaultdict
the script fills, and the non-conspecific genomes are printed in full by a second pass with acceptPer = -1, where every tree is
"filtered".  Sums and columns follow first appearance among the leaves (the dicts of the running Python 3); str(float) is Python 3's.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_genetrees_golden.py [--time]      (writes tests/golden/genetrees_cases.json;
       --time: the reference's two loops on one core over a synthetic forest, to profiles/r26_genetrees_reference_cpu.json)"""
import ast
import builtins
import contextlib
import io
import json
import os
import random
import re
import shutil
import sys
import tempfile
import time
import types
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))

import dendropy as shim                                                                                                  # noqa: E402
from checkm_amd.genomeTree import GenomeTree                                                                             # noqa: E402
from tools.gen_simulation_golden import translate                                                                        # noqa: E402

PRINTS = ("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)")
PARALOG_SUBSTITUTIONS = [PRINTS, ("xrange", r"\bxrange\(", "range("), ("iteritems", r"\.iteritems\(\)", ".items()")]
PARALOG_HITS = {"print statements": 12, "xrange": 2, "iteritems": 1}
CONSISTENCY_SUBSTITUTIONS = [PRINTS, ("xrange", r"\bxrange\(", "range("), ("iteritems", r"\.iteritems\(\)", ".items()")]
CONSISTENCY_HITS = {"print statements": 8, "xrange": 9, "iteritems": 1}
TIGR_DIR, PFAM_FILE = "/srv/db/tigrfam/13.0/TIGRFAMs_13.0_INFO", "/srv/db/pfam/27/Pfam-A.clans.tsv"


# ---- the dendropy stand-in ---------------------------------------------------------------------------------------------------------------
class GNode(shim.Node):
    def distance_from_root(self):
        if self.parent_node is None:
            return float(self.edge_length) if self.edge_length is not None else 0.0
        d = float(self.edge_length)
        p = self.parent_node
        while p is not None:
            if p.edge_length is not None:
                d = d + float(p.edge_length)
            p = p.parent_node
        return d


class GTree(shim.Tree):
    @classmethod
    def get_from_path(cls, src, schema, **kwargs):
        kwargs.pop("as_rooted", None)
        with open(src) as f:
            tree = cls.get_from_string(f.read(), schema, **kwargs)
        adopt(tree)
        return tree

    def mrca(self, taxon_labels):
        want = set(taxon_labels)
        common = None
        for leaf in self.leaf_nodes():
            if leaf.taxon.label in want:
                path, v = [], leaf
                while v is not None:
                    path.append(v)
                    v = v.parent_node
                common = path if common is None else [x for x in common if any(x is y for y in path)]
        internal = [v for v in common if v.is_internal()]
        return internal[0] if internal else common[0]


def adopt(tree):
    for v in tree.seed_node.preorder_iter():
        v.__class__ = GNode


def genome_of(label):
    return label[4:] if label.startswith("IMG_") else label.split("|")[0] if "|" in label else label


def make_reroot(metadata):
    class RerootTree(object):
        def reroot(self, tree):
            old = {v.taxon.label: v for v in tree.leaf_nodes()}
            outgroup = [label for label in old if metadata[genome_of(label)]["taxonomy"][0].lower() == "archaea"]
            fresh = GTree.get_from_string(GenomeTree.reroot(tree.as_string(schema="newick"), outgroup), "newick", preserve_underscores=True)
            adopt(fresh)
            for leaf in fresh.leaf_nodes():                       # the script took its leaf objects before the call: they stay the leaves
                mine, parent = old[leaf.taxon.label], leaf.parent_node
                parent._children[[k for k, c in enumerate(parent._children) if c is leaf][0]] = mine
                mine.parent_node, mine.edge_length = parent, leaf.edge_length
            tree.seed_node = fresh.seed_node
    return RerootTree


# ---- the scripts' surroundings -----------------------------------------------------------------------------------------------------------
def surroundings(case_dir, copies):
    def real(path):
        if path.startswith(TIGR_DIR):
            return os.path.join(case_dir, "tigrfam_info") + path[len(TIGR_DIR):]
        return os.path.join(case_dir, "Pfam-A.clans.tsv") if path == PFAM_FILE else path

    def system(cmd):
        words = cmd.split(" ")
        if len(words) != 3 or words[0] != "cp":
            raise SystemExit("unexpected command: %r" % cmd)
        shutil.copyfile(words[1], words[2])
        copies.append(os.path.basename(words[2]))

    os_stand = types.SimpleNamespace(path=os.path, makedirs=os.makedirs, remove=os.remove, listdir=lambda p: sorted(os.listdir(real(p))), system=system)
    return os_stand, (lambda path, *a: builtins.open(real(path), *a))


def load_class(source, script, name, substitutions, hits, names):
    text = open(os.path.join(source, "scripts", "genometreeworkflow", script)).read()
    m = re.search(r"(?ms)^class %s\(object\):.*?(?=^if __name__)" % name, text)
    if not m:
        raise SystemExit("class %s not found in %s" % (name, script))
    ns = dict(names)
    exec(compile(translate(m.group(0), substitutions, hits), "<%s, translated in memory>" % script, "exec"), ns)
    return ns[name]


def write_case(case):
    d = tempfile.mkdtemp(prefix="ckm_genetrees_golden_")
    os.makedirs(os.path.join(d, "trees"))
    os.makedirs(os.path.join(d, "tigrfam_info"))
    for name, text in case["trees"].items():
        open(os.path.join(d, "trees", name), "w").write(text)
    for name, text in case["tigrfam_info"].items():
        open(os.path.join(d, "tigrfam_info", name), "w").write(text)
    open(os.path.join(d, "Pfam-A.clans.tsv"), "w").write(case["pfam_clans"])
    return d


def metadata_of(case):
    return {row[0]: {"taxonomy": row[1:8]} for row in case["metadata"]}


def run_paralog(source, case, d, accept):
    metadata, copies, made = metadata_of(case), [], []

    def recording(factory):
        made.append(defaultdict(factory))
        return made[-1]

    os_stand, open_stand = surroundings(d, copies)
    img = lambda *_: types.SimpleNamespace(genomeMetadata=lambda: metadata)
    Paralog = load_class(source, "paralogTest.py", "ParalogTest", PARALOG_SUBSTITUTIONS, PARALOG_HITS,
                         dict(os=os_stand, open=open_stand, IMG=img, dendropy=types.SimpleNamespace(Tree=GTree), RerootTree=make_reroot(metadata), defaultdict=recording))
    out_dir = os.path.join(d, "conspecific_%s" % ("all" if accept < 0 else "kept"))
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        Paralog().run(os.path.join(d, "trees"), accept, case["extension"], out_dir)
    return text.getvalue(), copies, [sorted(x.keys()) for x in made], sorted(os.listdir(out_dir))


def paralog_expected(source, case, d):
    text, copies, paralogs, kept = run_paralog(source, case, d, case["acceptPer"])
    full, _, _, _ = run_paralog(source, case, d, -1.0)
    ids = re.findall(r"(?m)^  Testing gene tree: (.*)$", text)
    sizes = [int(x) for x in re.findall(r"(?m)^  Genes in tree: (\d+)$", text)]
    lists = [sorted(ast.literal_eval(x)) for x in re.findall(r"(?m)^  Tree is not conspecific for the following genome: (.*)$", full)]
    files = [f for f in sorted(case["trees"]) if f.endswith(case["extension"])]
    if not (len(ids) == len(sizes) == len(lists) == len(paralogs) == len(files)) or sorted(copies) != kept:
        raise SystemExit("the paralog passes do not line up")
    return {"records": [{"geneId": i, "numTaxa": n, "paralogs": p, "nonConspecific": q, "retained": f in kept} for i, n, p, q, f in zip(ids, sizes, paralogs, lists, files)],
            "copied": kept}


def consistency_expected(source, case, d):
    metadata, copies = metadata_of(case), []
    os_stand, open_stand = surroundings(d, copies)
    img = lambda *_: types.SimpleNamespace(genomeMetadata=lambda: metadata)
    Consistency = load_class(source, "consistencyTest.py", "ConsistencyTest", CONSISTENCY_SUBSTITUTIONS, CONSISTENCY_HITS,
                             dict(os=os_stand, open=open_stand, sys=sys, IMG=img, dendropy=types.SimpleNamespace(Tree=GTree)))
    out_dir, out_file = os.path.join(d, "final"), os.path.join(d, "consistency.tsv")
    with contextlib.redirect_stdout(io.StringIO()):
        Consistency().run(os.path.join(d, "trees"), case["extension"], case["consistencyThreshold"], case["minTaxaForAverage"], out_file, out_dir)
    per_tree = {f: open(os.path.join(out_dir, "consistency", f)).read() for f in sorted(os.listdir(os.path.join(out_dir, "consistency")))}
    kept = sorted(f for f in os.listdir(out_dir) if os.path.isfile(os.path.join(out_dir, f)))
    if sorted(copies) != kept:
        raise SystemExit("the copies of the consistency pass do not line up")
    return {"results": per_tree, "table": open(out_file).read(), "copied": kept}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def taxonomy_rows():
    rows = []

    def add(g, *tax):
        rows.append([g] + list(tax))
    add("B1", "Bacteria", "Proteobacteria", "Gammaproteobacteria", "Enterobacterales", "Enterobacteriaceae", "Escherichia", "Coli")
    add("B2", "Bacteria", "Proteobacteria", "Gammaproteobacteria", "Enterobacterales", "Enterobacteriaceae", "Escherichia", "coli")
    add("B3", "Bacteria", "Proteobacteria", "Gammaproteobacteria", "Enterobacterales", "Enterobacteriaceae", "Salmonella", "enterica")
    add("B4", "Bacteria", "Proteobacteria", "Alphaproteobacteria", "Rhizobiales", "Rhizobiaceae", "Rhizobium", "unclassified")
    add("B5", "Bacteria", "Proteobacteria", "Alphaproteobacteria", "Rhizobiales", "Rhizobiaceae", "unclassified", "sp. X")
    add("B6", "Bacteria", "Firmicutes", "Bacilli", "Bacillales", "Bacillaceae", "Bacillus", "subtilis")
    add("B7", "Bacteria", "Firmicutes", "Bacilli", "Bacillales", "Bacillaceae", "Bacillus", "")
    add("B8", "Bacteria", "Firmicutes", "Clostridia", "Clostridiales", "Clostridiaceae", "Clostridium", "difficile")
    add("B9", "Bacteria", "unclassified", "unclassified", "unclassified", "unclassified", "unclassified", "unclassified")
    add("B10", "Bacteria", "Firmicutes", "unclassified", "unclassified", "unclassified", "unclassified", "unclassified")
    add("A1", "Archaea", "Euryarchaeota", "Methanococci", "Methanococcales", "Methanococcaceae", "Methanococcus", "maripaludis")
    add("A2", "Archaea", "Euryarchaeota", "Methanococci", "Methanococcales", "Methanococcaceae", "Methanococcus", "vannielii")
    add("A3", "Archaea", "Crenarchaeota", "Thermoprotei", "Sulfolobales", "Sulfolobaceae", "Sulfolobus", "solfataricus")
    return rows


def random_tree(rnd, genomes, copies, zero=0.2):
    """A Newick text over one gene per genome and `copies` extra genes, with multifurcations, single-child nodes and zero lengths."""
    labels = ["%s|g%d" % (g, k) for k, g in enumerate(genomes)] + ["%s|x%d" % (rnd.choice(genomes), k) for k in range(copies)]
    rnd.shuffle(labels)
    length = lambda: "0.0" if rnd.random() < zero else repr(round(rnd.random() * 0.5, 4))
    nodes = [lab + ":" + length() for lab in labels]
    while len(nodes) > 1:
        k = min(len(nodes), rnd.choice((2, 2, 2, 3, 4)))
        at = rnd.randrange(len(nodes) - k + 1)
        joined = "(" + ",".join(nodes[at:at + k]) + ")"
        if len(nodes) > k:
            joined += ":" + length()
            if rnd.random() < 0.15:
                joined = "(" + joined + "):" + length()
        nodes[at:at + k] = [joined]
    return nodes[0] + ";\n"


def cases():
    rows = taxonomy_rows()
    genomes = [r[0] for r in rows]
    rnd = random.Random(28)
    info = {"TIGR00003.INFO": "ID  three\nAC  TIGR00003\nDE  third family\nCC  a longer text  with two spaces\n", "TIGR00005.INFO": "AC  TIGR00005\nDE  fifth family\n"}
    clans = "PF00001\tCL0001\tclan\tshortA\tlong description A\nPF00002\t\t\tshortB\tlong B\nPF00004\t\t\tshortD\tlong D\nPF00006\t\t\tshortF\tlong F\n"
    hand = {
        # archaea on one edge; B1 twice as neighbours (conspecific); B6 twice at distance 0 (no paralog)
        "PF00001.tre": "((A1|a:0.2,(A2|a:0.1,A3|a:0.3):0.05):0.4,((B1|a:0.1,B1|b:0.12):0.05,B2|a:0.2):0.1,((B6|a:0.0,B6|b:0.0):0.2,(B7|a:0.1,B8|a:0.3):0.1):0.2,(B3|a:0.2,B4|a:0.1):0.3);\n",
        # B1's copies enclose Salmonella and Bacillus: not conspecific; B4's enclose only leaves that are not counted
        "PF00002.tre": "((B1|a:0.1,B3|a:0.2):0.1,(B6|a:0.3,B1|b:0.2):0.1,(B4|a:0.1,(B5|a:0.1,(B9|a:0.2,B4|b:0.1):0.1):0.1):0.2,(A1|a:0.5,B8|a:0.2):0.3);\n",
        # a star: every common ancestor is the root; two genomes with three copies, some at distance 0
        "TIGR00003.tre": "(B1|a:0.0,B1|b:0.0,B1|c:0.1,B2|a:0.0,B2|b:0.0,B3|a:0.2,A1|a:0.3,A1|b:0.0);\n",
        # the name maps pfam -> PF; chains of single-child nodes, a quoted label, five copies of B8
        "pfam00004.tre": "(((B8|a:0.1):0.0):0.1,((B8|b:0.0,B8|c:0.0):0.0,('B8|d':0.1,B8|e:0.2):0.1):0.1,((B6|a:0.2,B7|a:0.1):0.1,(A2|a:0.3):0.2):0.1);\n",
        "TIGR00005.tre": random_tree(rnd, genomes, 9),
        "PF00006.tre": random_tree(rnd, genomes[:8], 5),
        "notes.txt": "not a tree\n",
        "PF00001.tre.bak": "not a tree either\n",
    }
    first = {"name": "thirteen_genomes", "metadata": rows, "trees": hand, "extension": ".tre", "acceptPer": 0.01, "consistencyThreshold": 0.5, "minTaxaForAverage": 1,
             "tigrfam_info": info, "pfam_clans": clans, "paralog": True}
    lenient = dict(first, name="lenient_defaults", acceptPer=0.2, consistencyThreshold=0.86, minTaxaForAverage=20)
    bare = {"PF00001.tree": "((IMG_A1:0.2,IMG_A2:0.1):0.4,(IMG_B1:0.1,(B2:0.12,B3|g:0.1):0.05):0.1,(IMG_B6:0.2,(IMG_B8:0.1,B7:0.3):0.1):0.2);\n",
            "PF00002.tree": "(IMG_B1:0.1,IMG_B6:0.2);\n", "TIGR00003.tree": "(IMG_B1:0.1,(IMG_A1:0.2,IMG_B2:0.1):0.1,IMG_A3:0.2);\n"}
    img_labels = dict(first, name="img_labels", trees=bare, extension=".tree", consistencyThreshold=0.3, minTaxaForAverage=1, paralog=False)
    return [first, lenient, img_labels]


def time_reference(source, ntrees=2, leaves=3000):
    """The forest of tools/genetrees_bench.py (same generator, same shape), fewer trees."""
    from tests import genetrees_synth as synth
    ngenomes = leaves * 3 // 4
    md = synth.metadata(ngenomes, nphyla=30, nclasses=60)
    metadata = [[g] + m["taxonomy"] for g, m in md.items()]
    genomes = list(md)
    trees = {name: text + "\n" for name, text in synth.forest(26, [("PF%05d.tre" % k, "random", leaves, ngenomes, (), 0.05) for k in range(ntrees)])}
    case = {"metadata": metadata, "trees": trees, "extension": ".tre", "acceptPer": 0.01, "consistencyThreshold": 0.86, "minTaxaForAverage": 20,
            "tigrfam_info": {}, "pfam_clans": "".join("PF%05d\t\t\ts\tl\n" % k for k in range(ntrees))}
    d = write_case(case)
    t0 = time.perf_counter()
    run_paralog(source, case, d, 0.01)
    t1 = time.perf_counter()
    consistency_expected(source, case, d)
    t2 = time.perf_counter()
    out = {"what": "the reference's paralogTest and consistencyTest loops (text translated in memory, the golden tool's dendropy stand-in), one core",
           "trees": len(trees), "leaves_per_tree": leaves, "genomes": len(genomes), "paralog_s": t1 - t0, "consistency_s": t2 - t1}
    path = os.path.join(ROOT, "profiles", "r26_genetrees_reference_cpu.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, sort_keys=True) + "\n")
    print(json.dumps(out, sort_keys=True))


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    if not os.path.isdir(os.path.join(source, "scripts", "genometreeworkflow")):
        raise SystemExit("set CHECKM_SOURCE to the CheckM source tree")
    if "--time" in sys.argv[1:]:
        return time_reference(source)
    out = []
    for case in cases():
        d = write_case(case)
        expected = {"paralog": paralog_expected(source, case, d) if case["paralog"] else None, "consistency": consistency_expected(source, case, d)}
        out.append(dict(case, expected=expected))
    path = os.path.join(ROOT, "tests", "golden", "genetrees_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
