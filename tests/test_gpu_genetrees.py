"""The gene-tree tests on the device: the kernels of libcheckm_hip (kernels_genetree.hip) against the host executor of the same header
(ckm_genetree_host) at == on the three outputs -- the bits of every consistency, every paralog flag, every common ancestor and
conspecific result -- on the smallest shapes that can still break: trees of 2 and of 3 leaves, leaf counts around the wavefront, the
256-leaf step of the scan and many steps of it, a caterpillar, a balanced tree, a star, one class over every leaf, a class per leaf,
single-child chains, five copies of a genome with some at distance 0, common ancestors at the root, species ranges without a counted
leaf; three budgets; the goldens through GeneTrees' default device path; and one run from alignments to the directory that
GenomeTree.concatenate takes.  Everywhere but in the refusals the count of trees that fell back to Python must be 0."""
import json
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib, geneTrees
from checkm_amd.geneTrees import GeneTrees
from checkm_amd.genomeTree import GenomeTree
from checkm_amd.img import IMG
from tests import genetrees_synth as synth
from tests.emu import genetrees as emu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "genetrees_cases.json")))
OUTPUTS = ("consistency", "pair_flag", "group_node", "group_mixed")


def shapes():
    """[(name, text)] and the metadata of the forest."""
    md = synth.metadata(3200)
    md.update(synth.metadata(200, one_class=True, prefix="O"))
    md.update(synth.metadata(257, distinct=True, prefix="E"))
    md.update(synth.metadata(40, uncounted=True, prefix="U"))
    specs = [("two", "random", 2, 2, (), 0.0), ("three", "star", 3, 2, ((0, 2),), 0.0)]
    specs += [("n%d" % n, "random", n, max(2, n * 3 // 4), ((1, 3),), 0.1) for n in (63, 64, 65, 257, 1025, 4097)]
    specs += [("caterpillar", "caterpillar", 300, 200, ((2, 3),), 0.1), ("balanced", "balanced", 256, 150, ((0, 2),), 0.1), ("star", "star", 130, 60, ((5, 4),), 0.4),
              ("one_class", "random", 200, 150, ((3, 2),), 0.1, "O"), ("class_per_leaf", "random", 257, 257, (), 0.1, "E"), ("chain", "chain", 100, 60, ((4, 3),), 0.2),
              ("five_copies", "random", 70, 50, ((1, 5),), 0.6), ("not_counted", "random", 90, 40, ((7, 4), (2, 3)), 0.1, "U")]
    return synth.forest(2810, specs), md


@pytest.fixture(scope="module")
def forest():
    trees, md = shapes()
    packed = [geneTrees.packTree(name, text, md, geneTrees.genomeIdOfGene) for name, text in trees]
    tables = geneTrees.forestTables(packed)
    want = _lib.genetree_host(tables)
    for f in OUTPUTS:
        want[f].setflags(write=False)
    return packed, tables, want


def test_forest_has_the_shapes_it_names(forest):
    packed, tables, want = forest
    by = {p.name: (k, p) for k, p in enumerate(packed)}
    assert [len(by[n][1].labels) for n in ("two", "three", "n63", "n64", "n65", "n257", "n1025", "n4097")] == [2, 3, 63, 64, 65, 257, 1025, 4097]
    assert int(by["three"][1].internal.sum()) == 1 and int(by["star"][1].internal.sum()) == 1
    assert [len(c) for c in by["one_class"][1].classes] == [1, 1, 1] and [len(c) for c in by["class_per_leaf"][1].classes] == [257, 257, 257]
    chain = by["chain"][1]
    children = np.bincount(chain.parent[1:], minlength=len(chain.parent))
    assert (children[chain.internal == 1] == 1).sum() > 10
    assert max(len(g) for g in by["five_copies"][1].pairs) >= 10
    assert (by["not_counted"][1].leaf_species == geneTrees.NONE).all()

    def groups(name):
        k = by[name][0]
        g0, g1 = int(tables.group_off[k]), int(tables.group_off[k + 1])
        return want["group_node"][g0:g1], want["group_mixed"][g0:g1], want["pair_flag"][int(tables.gpair_off[g0]):int(tables.gpair_off[g1])]

    node, mixed, flags = groups("five_copies")
    assert flags.any() and not flags.all()                            # some copies at distance 0
    node, mixed, flags = groups("star")
    assert (node[node != geneTrees.NONE] == 0).all() and (node == 0).any()            # a paralog set whose common ancestor is the root
    node, mixed, flags = groups("not_counted")
    assert flags.any() and not mixed.any()
    assert want["group_mixed"].any() and (want["group_node"] == geneTrees.NONE).any()


def test_device_equals_host_executor_under_three_budgets(gpu_ctx, forest):
    packed, tables, want = forest
    sizes = [emu.tree_bytes(tables, k) for k in range(tables.ntrees)]
    rounds = set()
    for budget in (1, sum(sizes) // 2, 1 << 30):
        got = _lib.genetree_run(gpu_ctx, tables, budget)
        assert got["consistency"].tobytes() == want["consistency"].tobytes(), budget
        for f in OUTPUTS:
            assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (budget, f)
        assert got["nrounds"] == emu.rounds(tables, budget) and got["ntrees"] == tables.ntrees
        rounds.add(got["nrounds"])
    assert tables.ntrees in rounds and 1 in rounds and len(rounds) == 3


def test_tree_tests_through_the_class_do_not_fall_back(gpu_ctx, forest):
    packed, tables, want = forest
    trees, md = shapes()
    res = GeneTrees().treeTests(trees, md, geneTrees.genomeIdOfGene)
    assert res["info"]["python_trees"] == 0 and res["info"]["ntrees"] == len(trees) and res["info"]["launches"] == 3
    for f in OUTPUTS:
        assert np.concatenate(res[f]).tolist() == want[f].tolist(), f


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_through_the_device(gpu_ctx, case, tmp_path):
    infos = synth.check_golden_case(GeneTrees(), case, str(tmp_path))
    assert all(i["python_trees"] == 0 and i["launches"] > 0 for i in infos)


def test_refusals_before_any_launch(gpu_ctx):
    many = synth.metadata((1 << 14) + 1, one_class=True)
    big = geneTrees.packTree("big", synth.newick("star", ["G%d|x" % k for k in range((1 << 14) + 1)], random.Random(1)), many)
    with pytest.raises(_lib.CkmError) as e:
        _lib.genetree_run(gpu_ctx, geneTrees.forestTables([big]))
    assert e.value.code == -7
    small = geneTrees.packTree("small", "(G1|a:0.1,(G1|b:0.2,G2|a:0.1):0.1);", many)
    t = geneTrees.forestTables([small])
    t.length[1] = np.nan
    with pytest.raises(_lib.CkmError) as e:
        _lib.genetree_run(gpu_ctx, t)
    assert e.value.code == -1
    res = GeneTrees().treeTests([("big", big_text()), ("small", "(G1|a:0.1,(G1|b:0.2,G2|a:0.1):0.1);")], many, geneTrees.genomeIdOfGene)
    assert res["info"]["python_trees"] == 1 and res["info"]["ntrees"] == 1 and res["consistency"][0].tolist() == [1.0, 1.0, 1.0]


def big_text():
    return synth.newick("star", ["G%d|x" % k for k in range((1 << 14) + 1)], random.Random(1))


METADATA_HEADER = ["taxon_oid", "Domain", "Status", "Phylum", "Class", "Order", "Family", "Genus", "Species", "Scaffold Count", "GC Count", "Genome Size", "Gene Count",
                   "Coding Base Count", "Biotic Relationships", "N50"]


def test_run_from_alignments_to_the_genome_tree_s_directory(gpu_ctx, tmp_path):
    rnd = random.Random(11)
    aa = "ARNDCQEGHILKMFPSTWYV"
    tax = {"A1": ["Archaea", "Euryarchaeota", "Methanococci"], "A2": ["Archaea", "Euryarchaeota", "Methanococci"], "B1": ["Bacteria", "Proteobacteria", "Gammaproteobacteria"],
           "B2": ["Bacteria", "Proteobacteria", "Gammaproteobacteria"], "B3": ["Bacteria", "Proteobacteria", "Gammaproteobacteria"], "B4": ["Bacteria", "Firmicutes", "Bacilli"],
           "B5": ["Bacteria", "Firmicutes", "Bacilli"], "B6": ["Bacteria", "Firmicutes", "Bacilli"]}
    d = tmp_path
    with open(str(d / "img_metadata.tsv"), "w") as f:
        f.write("\t".join(METADATA_HEADER) + "\n")
        for g, t in tax.items():
            f.write("\t".join([g, t[0], "Finished", t[1], t[2], "O", "F", "Genus" + t[2], "species " + t[2], "1", "5000", "10000", "10", "9000", "Free living", "10000"]) + "\n")
    (d / "tigrfam2pfam.tsv").write_text("")
    (d / "aln").mkdir()

    def mutate(seq, n):
        s = list(seq)
        for k in rnd.sample(range(len(s)), n):
            s[k] = rnd.choice(aa)
        return "".join(s)

    hits = {g: ([], []) for g in tax}
    for gene, family, tigr in (("PF00001", "pfam00001", False), ("TIGR00002", "TIGR00002", True)):
        base = "".join(rnd.choice(aa) for _ in range(120))
        clade = {c: mutate(base, 50) for c in ("Methanococci", "Gammaproteobacteria", "Bacilli")}
        records = []
        for g, t in tax.items():
            copies = ["a", "b"] if (g == "B2" and not tigr) else ["a"]
            own = mutate(clade[t[2]], 8)
            for c in copies:
                gene_id = g + "_" + gene + c
                records.append(">%s|%s\n%s*\n" % (g, gene_id, mutate(own, 1 if c == "b" else 0)))
                if tigr:
                    hits[g][1].append("\t".join([gene_id, "300", "50.0", "1", "1e-20", "x", family, "name"]) + "\n")
                else:
                    hits[g][0].append("\t".join([gene_id, "300", "50.0", "1", "100", "1", "1e-20", "x", family, "name"]) + "\n")
        (d / "aln" / (gene + ".aln.masked.faa")).write_text("".join(records))
    for g in tax:
        (d / "genomes" / g).mkdir(parents=True)
        (d / "genomes" / g / (g + IMG.pfamExtension)).write_text("header\n" + "".join(hits[g][0]))
        (d / "genomes" / g / (g + IMG.tigrExtension)).write_text("header\n" + "".join(hits[g][1]))
    img = IMG(str(d / "img_metadata.tsv"), str(d / "tigrfam2pfam.tsv"), str(d / "genomes"))
    gt = GeneTrees()
    final = gt.run(str(d / "aln"), str(d / "work"), img.genomeMetadata(), {"PF00001": ["s1", "l1"], "TIGR00002": ["s2", "l2"]}, consistencyThreshold=0.5, minTaxaForAverage=1)
    assert gt.lastInfo["python_trees"] == 0 and gt.lastInfo["launches"] > 0
    assert sorted(os.listdir(final)) == ["PF00001.aln.masked.tre", "TIGR00002.aln.masked.tre", "consistency"]
    assert "*" not in (d / "aln" / "PF00001.aln.masked.faa").read_text().replace(">", "")
    seqs = GenomeTree().concatenate(final, str(d / "aln"), ".aln.masked.faa", str(d / "out.faa"), str(d / "out.tax"), img)
    assert sorted(seqs) == sorted("IMG_" + g for g in tax) and set(len(s) for s in seqs.values()) == {242}
