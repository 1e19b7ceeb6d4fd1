"""DecorateTree without a device (buildMarkerSets through the host executor of tests/emu/markerset): a 12-leaf tree with duplicates and a
taxa tree; the labels UID<n>|<taxonomy>|<bootstrap> in pre-order, with the empty taxonomy and the empty bootstrap; the table read back by
both readNodeMetadata; the marker column against buildMarkerSet of each node's genomes; mean and std strings against numpy's on the same
values with 'NA' skipped; the Pfam accession mapping; and buildBinMarkerSet walking the decorated tree."""
import os

import numpy as np
import pytest

from checkm_amd.decorateTree import DecorateTree, internalNodes, mrca, setLiteral
from checkm_amd.defaultValues import DefaultValues
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from checkm_amd.treeParser import Tree, TreeParser, parse_set_literal, read_newick
from tests.test_markerset_host import use_host_executor

INPUT_TREE = ("(((IMG_1:0.1,IMG_2:0.1)0.95:0.1,(IMG_3:0.1,IMG_4:0.2):0.1)0.80:0.2,((IMG_5:0.1,IMG_6:0.1)1.000:0.1,(IMG_7:0.1,(IMG_8:0.1,IMG_9:0.1)0.5:0.1)0.7:0.1)0.9:0.1,"
              "(IMG_10:0.1,(IMG_11:0.1,IMG_12:0.1)0.6:0.1)0.65:0.3);\n")
TAXA_TREE = ("(((IMG_1,IMG_101,IMG_102,IMG_2)'g__Alpha beta',(IMG_3,IMG_4))'p__Proteo bacteria',((IMG_5,IMG_6)f__Fam,(IMG_7,(IMG_8,IMG_108,IMG_9)))c__Cls,IMG_10)"
             "'k__Bacteria';\n")
DEREP = "IMG_1 IMG_101 IMG_102\nIMG_8\tIMG_108\nIMG_5\n"
GENOMES = [str(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 101, 102, 108)]
# what each node must get: (leaves and their duplicates in order, taxonomy, bootstrap)
NODES = [
    (["1", "101", "102", "2", "3", "4", "5", "6", "7", "8", "108", "9", "10", "11", "12"], "k__Bacteria", ""),
    (["1", "101", "102", "2", "3", "4"], "p__Proteobacteria", "0.80"),
    (["1", "101", "102", "2"], "g__Alphabeta", "0.95"),
    (["3", "4"], "", ""),
    (["5", "6", "7", "8", "108", "9"], "c__Cls", "0.9"),
    (["5", "6"], "f__Fam", "1.000"),
    (["7", "8", "108", "9"], "", "0.7"),
    (["8", "108", "9"], "", "0.5"),
    (["10", "11", "12"], "", "0.65"),                                                  # only IMG_10 is in the taxa tree: a leaf has no label
    (["11", "12"], "", "0.6"),                                                         # none of its labels is in the taxa tree
]


class FakeIMG(object):
    """What MarkerSetBuilder and DecorateTree ask of the IMG reader, from tables in memory."""
    FAMILIES = {"pfam00001": 1000, "pfam00002": 3000, "pfam00003": 50000, "pfam00004": 200000, "pfam00005": 100000, "pfam00006": 102000, "TIGR00001": 300000}

    def __init__(self):
        self.counts = {f: {g: 1 for g in GENOMES} for f in self.FAMILIES}
        for g in ("5", "6", "7", "8", "9", "108"):
            del self.counts["pfam00003"][g]
        self.counts["pfam00004"]["3"] = 2
        del self.counts["TIGR00001"]["11"]

    def genomeMetadata(self):
        md = {}
        for k, g in enumerate(GENOMES):
            md[g] = {"GC %": 0.3 + 0.013 * k, "genome size": 1500000 + 77777 * k, "gene count": 1400 + 91 * k, "taxonomy": ["Bacteria"] + ["x"] * 6}
        md["2"]["gene count"] = "NA"
        md["3"]["GC %"] = "NA"
        md["4"]["GC %"] = "NA"
        md["102"]["genome size"] = "NA"
        return md

    def geneCountTable(self, genomeIds):
        return {f: {g: c for g, c in counts.items() if g in set(genomeIds)} for f, counts in self.counts.items()}

    def geneDistTable(self, genomeIds, markerGenes, spacingBetweenContigs=0):
        return {g: {m: [(self.FAMILIES[m] + 10 * k, self.FAMILIES[m] + 10 * k + 900) for k in range(self.counts[m][g])] for m in markerGenes if g in self.counts.get(m, {})}
                for g in genomeIds}

    def identifyRedundantTIGRFAMs(self, markerGenes):
        return set()


@pytest.fixture()
def decorated(tmp_path, monkeypatch):
    use_host_executor(monkeypatch)
    paths = {k: str(tmp_path / k) for k in ("taxa.tre", "genome_tree.derep.txt", "genome_tree.final.tre", "genome_tree.metadata.tsv")}
    open(paths["taxa.tre"], "w").write(TAXA_TREE)
    open(paths["genome_tree.derep.txt"], "w").write(DEREP)
    open(paths["genome_tree.final.tre"], "w").write(INPUT_TREE)
    img = FakeIMG()
    rows = DecorateTree(img).decorate(paths["taxa.tre"], paths["genome_tree.derep.txt"], paths["genome_tree.final.tre"], paths["genome_tree.metadata.tsv"])
    return img, paths, rows


def test_labels_in_preorder_with_the_empty_cases(decorated):
    img, paths, rows = decorated
    tree = Tree.from_path(paths["genome_tree.final.tre"])
    labels = [v.label for v in internalNodes(tree)]
    assert labels == ["UID%d|%s|%s" % (k, taxa, boot) for k, (_, taxa, boot) in enumerate(NODES, 1)]
    assert labels[3] == "UID4||" and labels[0] == "UID1|k__Bacteria|" and labels[6] == "UID7||0.7"
    assert [leaf.taxon for leaf in tree.root.leaves()] == ["IMG_%d" % k for k in range(1, 13)]
    before, after = read_newick(INPUT_TREE), tree
    assert [leaf.length for leaf in before.root.leaves()] == [leaf.length for leaf in after.root.leaves()]
    assert [r["labels"] for r in rows] == [["IMG_" + g for g in ids] for ids, _, _ in NODES]
    taxa = read_newick(TAXA_TREE)
    assert mrca(taxa, ["IMG_11", "nobody"]) is None and mrca(taxa, ["IMG_8", "IMG_7", "absent"]).label == "" and mrca(taxa, ["IMG_5", "IMG_9"]).label == "c__Cls"


def test_table_is_read_back_by_both_readers(decorated, monkeypatch, tmp_path):
    img, paths, rows = decorated
    text = open(paths["genome_tree.metadata.tsv"]).read().split("\n")
    assert text[0] == "UID\t# genomes\tTaxonomy\tBootstrap\tGC mean\tGC std\tGenome size mean\tGenome size std\tGene count mean\tGene count std\tMarker set"
    assert [ln.split("\t")[0] for ln in text[1:-1]] == ["UID%d" % k for k in range(1, 11)] and text[-1] == ""
    b = MarkerSetBuilder(img)
    mine = b.readNodeMetadata(paths["genome_tree.metadata.tsv"])
    os.makedirs(tmp_path / "data" / "genome_tree")
    open(tmp_path / "data" / "genome_tree" / "genome_tree.metadata.tsv", "w").write("\n".join(text))
    monkeypatch.setattr(DefaultValues, "CHECKM_DATA_DIR", str(tmp_path / "data"))
    theirs = TreeParser().readNodeMetadata()
    assert repr(mine) == repr(theirs) and sorted(mine) == sorted("UID%d" % k for k in range(1, 11))
    for k, (ids, taxa, boot) in enumerate(NODES, 1):
        d = mine["UID%d" % k]
        assert d["# genomes"] == len(ids) and d["taxonomy"] == taxa and d["bootstrap"] == (float(boot) if boot else "NA")


def test_mean_and_std_strings_are_numpys_with_na_skipped(decorated):
    img, paths, rows = decorated
    md = img.genomeMetadata()
    lines = open(paths["genome_tree.metadata.tsv"]).read().split("\n")[1:-1]
    for line, (ids, _, _) in zip(lines, NODES):
        f = line.split("\t")
        gc = [md[g]["GC %"] for g in ids if md[g]["GC %"] != "NA"]
        size = [md[g]["genome size"] for g in ids if md[g]["genome size"] != "NA"]
        genes = [md[g]["gene count"] for g in ids if md[g]["gene count"] != "NA"]
        want = [str(np.mean(gc) * 100), str(np.std(gc) * 100), str(np.mean(size)), str(np.std(size)), str(np.mean(genes)), str(np.std(genes))] if gc else None
        if gc:
            assert f[4:10] == want
        else:
            assert f[4:6] == ["nan", "nan"] and f[6:10] == [str(np.mean(size)), str(np.std(size)), str(np.mean(genes)), str(np.std(genes))]
        assert "np." not in line
    assert len([md[g] for g in NODES[3][0] if md[g]["GC %"] != "NA"]) == 0 and len([g for g in NODES[2][0] if md[g]["gene count"] == "NA"]) == 1


def test_marker_column_is_buildMarkerSet_of_each_nodes_genomes(decorated):
    img, paths, rows = decorated
    b = MarkerSetBuilder(img)
    stats = b.readNodeMetadata(paths["genome_tree.metadata.tsv"])
    seen = set()
    for k, (ids, _, _) in enumerate(NODES, 1):
        got = parse_set_literal(stats["UID%d" % k]["marker set"])
        want = MarkerSetBuilder(img).buildMarkerSet(ids, 0.97, 0.97).markerSet
        assert sorted(sorted(s) for s in got) == sorted(sorted(s) for s in want) and got
        seen.add(stats["UID%d" % k]["marker set"])
    assert len(seen) > 2                                                               # the nodes do not all share one marker set
    assert {"pfam00001", "pfam00002"} in parse_set_literal(stats["UID1"]["marker set"])
    assert not any("pfam00003" in s for s in parse_set_literal(stats["UID5"]["marker set"])) and any("pfam00003" in s for s in parse_set_literal(stats["UID3"]["marker set"]))
    assert setLiteral([{"b", "a"}, set(), {"c"}]) == "[set(['a', 'b']), set([]), set(['c'])]"
    assert parse_set_literal(setLiteral([{"b", "a"}, {"c"}])) == [{"a", "b"}, {"c"}] and parse_set_literal(setLiteral([])) == []


def test_pfam_ids_become_accessions_and_are_dropped_when_absent(tmp_path, monkeypatch):
    use_host_executor(monkeypatch)
    for name, text in (("taxa.tre", TAXA_TREE), ("derep.txt", DEREP), ("in.tre", INPUT_TREE)):
        open(tmp_path / name, "w").write(text)
    open(tmp_path / "Pfam-A.hmm", "w").write("".join("HMMER3/f\nNAME  fam%d\nACC   PF0000%d.%d\nDESC  ACCessory text\n//\n" % (k, k, 10 + k) for k in (1, 2, 4, 5, 6)))
    img = FakeIMG()
    rows = DecorateTree(img, pfamHMMs=str(tmp_path / "Pfam-A.hmm")).decorate(str(tmp_path / "taxa.tre"), str(tmp_path / "derep.txt"), str(tmp_path / "in.tre"), str(tmp_path / "md.tsv"))
    stats = MarkerSetBuilder(img).readNodeMetadata(str(tmp_path / "md.tsv"))
    sets = parse_set_literal(stats["UID3"]["marker set"])
    members = set(m for s in sets for m in s)
    assert {"PF00001.11", "PF00002.12"} in sets and "TIGR00001" in members and not any(m.startswith("pfam") or m.startswith("PF00003") for m in members)
    assert rows[2]["markerSet"] == sets or sorted(map(sorted, rows[2]["markerSet"])) == sorted(map(sorted, sets))


def test_buildBinMarkerSet_walks_the_decorated_tree(decorated):
    img, paths, rows = decorated
    b = MarkerSetBuilder(img)
    b.readDuplicateSeqs(paths["genome_tree.derep.txt"])
    stats = b.readNodeMetadata(paths["genome_tree.metadata.tsv"])
    b.lineageSpecificGenesToRemove = {uid: set() for uid in stats}
    assert b.duplicateSeqs == {"IMG_1": ["IMG_101", "IMG_102"], "IMG_8": ["IMG_108"]}
    tree = Tree.from_path(paths["genome_tree.final.tre"])
    node = tree.find_leaf("IMG_8").parent
    binMarkerSets, refined = b.buildBinMarkerSet(tree, node, 0.97, 0.97)
    assert [ms.lineageStr for ms in binMarkerSets.markerSets] == ["UID8 | c__Cls", "UID7 | c__Cls", "UID5 | c__Cls", "UID1 | k__Bacteria"]
    assert [ms.numGenomes for ms in binMarkerSets.markerSets] == [3, 4, 6, 15]
    for ms, (ids, _, _) in zip(binMarkerSets.markerSets, (NODES[7], NODES[6], NODES[4], NODES[0])):
        want = parse_set_literal(stats[ms.lineageStr.split(" | ")[0]]["marker set"])
        assert sorted(sorted(s) for s in ms.markerSet) == sorted(sorted(s) for s in want)
    loo = b.buildBinMarkerSetsLOO(tree, ["2"], 0.97, 0.97)
    assert [ms.numGenomes for ms in loo["2"][0].markerSets] == [3, 5, 14]
