"""GeneTrees without a device: the emulator (tests/emu/genetrees.py) and GeneTrees(runner=emulator) against the goldens of the reference's
paralogTest.py and consistencyTest.py (tools/gen_genetrees_golden.py), the emulator against a brute force over explicit leaf sets, the
host executor ckm_genetree_host against the emulator at == under three budgets, makeTrees with a stand-in for `infer`, and the refusals
with the Python loop that runs in the library's place."""
import json
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib, geneTrees
from checkm_amd.geneTrees import GeneTrees
from checkm_amd.pplacer import parse_newick, plain_name
from tests import genetrees_synth as synth
from tests.emu import genetrees as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "genetrees_cases.json")))
OUTPUTS = ("consistency", "pair_flag", "group_node", "group_mixed")


def host_runner(tables, budget_bytes=0):
    return _lib.genetree_host(tables, budget_bytes)


@pytest.mark.parametrize("runner", [emu.runner, host_runner], ids=["emulator", "host_executor"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_byte_for_byte(case, runner, tmp_path):
    infos = synth.check_golden_case(GeneTrees(runner=runner), case, str(tmp_path))
    assert all(i["python_trees"] == 0 and i["ntrees"] == sum(f.endswith(case["extension"]) for f in case["trees"]) for i in infos)


def seeded_forest():
    md = synth.metadata(23)
    specs = [("r%d" % k, "random", n, 23, copies, zero) for k, (n, copies, zero) in
             enumerate([(31, ((1, 3), (4, 2)), 0.3), (40, ((0, 5), (2, 2), (9, 3)), 0.2), (17, ((6, 2),), 0.6), (29, ((3, 4), (5, 2)), 0.0), (2, (), 0.0), (3, ((7, 3),), 0.5)])]
    specs += [("chain", "chain", 21, 9, ((2, 3), (8, 2)), 0.3), ("star", "star", 12, 5, (), 0.5), ("cat", "caterpillar", 19, 7, ((1, 2),), 0.2), ("bal", "balanced", 33, 11, ((0, 2),), 0.1)]
    return synth.forest(2028, specs), md


def brute_force(text, p):
    """The three outputs of one tree from explicit leaf sets per node: no ranges, no prefix sums."""
    root = parse_newick(text)
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(reversed(v.children))
    number = {id(v): k for k, v in enumerate(order)}
    leaves = [v for v in order if not v.children]
    position = {id(v): k for k, v in enumerate(leaves)}
    assert [plain_name(v.name) for v in leaves] == p.labels
    below, depth = {}, {}
    for v in reversed(order):
        below[id(v)] = frozenset([position[id(v)]]) if not v.children else frozenset().union(*[below[id(c)] for c in v.children])
    for v in order:
        depth[id(v)] = 0 if v.parent is None else depth[id(v.parent)] + 1
    internal = [v for v in order if v.children]
    N = len(leaves)
    consistency = []
    for r in range(3):
        for c, T in enumerate(p.totals[r]):
            members = frozenset(k for k in range(N) if p.leaf_class[r, k] == c)
            assert len(members) == T
            best = 0
            for v in internal:
                k, n = len(below[id(v)] & members), len(below[id(v)])
                best = max(best, float(k) / (T + (n - k)), float(T - k) / (T + (N - n - (T - k))))
            consistency.append(best)

    def over(want):                                                   # the smallest subtree over the leaves; of equal sets the deepest
        return min((v for v in internal if want <= below[id(v)]), key=lambda v: (len(below[id(v)]), -depth[id(v)]))

    def length(v):
        return float(v.length) if v.length is not None else 0.0

    flags, nodes, mixed = [], [], []
    for pairs in p.pairs:
        flagged = set()
        for a, b in pairs:
            m, x, y = over({a, b}), leaves[a], leaves[b]
            if m.parent is None:
                total = []
                for v in (x, y):
                    d = length(v)
                    while v.parent is not None:
                        v = v.parent
                        d += length(v)
                    total.append(d)
                dist = total[0] + total[1]
            else:
                dist, v = length(x), x.parent
                while v is not m:
                    dist, v = dist + length(v), v.parent
                dist, v = dist + length(y), y.parent
                while v is not m:
                    dist, v = dist + length(v), v.parent
            flags.append(1 if dist > 0 else 0)
            if dist > 0:
                flagged |= {a, b}
        if flagged:
            m = over(flagged)
            nodes.append(number[id(m)])
            mixed.append(1 if len(set(int(p.leaf_species[k]) for k in below[id(m)]) - {geneTrees.NONE}) > 1 else 0)
        else:
            nodes.append(geneTrees.NONE)
            mixed.append(0)
    return consistency, flags, nodes, mixed


def test_emulator_equals_brute_force_over_leaf_sets():
    trees, md = seeded_forest()
    res = GeneTrees(runner=emu.runner).treeTests(trees, md, geneTrees.genomeIdOfGene)
    assert res["info"]["python_trees"] == 0
    seen_flag, seen_zero, seen_mixed, seen_root = False, False, False, False
    for k, (name, text) in enumerate(trees):
        want = brute_force(text, res["packed"][k])
        for f, w in zip(OUTPUTS, want):
            assert res[f][k].tolist() == list(w), (name, f)
        seen_flag |= bool(res["pair_flag"][k].any())
        seen_zero |= bool((res["pair_flag"][k] == 0).any())
        seen_mixed |= bool(res["group_mixed"][k].any())
        seen_root |= bool((res["group_node"][k] == 0).any())
    assert seen_flag and seen_zero and seen_mixed and seen_root          # the forest reaches every branch


def test_host_executor_equals_emulator_under_three_budgets():
    trees, md = seeded_forest()
    packed = [geneTrees.packTree(name, text, md, geneTrees.genomeIdOfGene) for name, text in trees]
    tables = geneTrees.forestTables(packed)
    want = emu.genetree_run(None, tables)
    sizes = [emu.tree_bytes(tables, k) for k in range(tables.ntrees)]
    seen = set()
    for budget in (1, 3 * max(sizes), 1 << 30):
        got = _lib.genetree_host(tables, budget)
        for f in OUTPUTS:
            assert np.array_equal(got[f], want[f]), (budget, f)
        assert got["consistency"].tobytes() == want["consistency"].tobytes()
        assert got["nrounds"] == emu.rounds(tables, budget) and got["ntrees"] == len(trees)
        seen.add(got["nrounds"])
    assert len(trees) in seen and 1 in seen and len(seen) == 3
    # the plain Python loop that stands in for a refused tree gives the same
    for k, p in enumerate(packed):
        c0, c1 = int(tables.class_off[3 * k]), int(tables.class_off[3 * k + 3])
        assert geneTrees.plainTreeTests(p)[0].tolist() == want["consistency"][c0:c1].tolist()


def test_make_trees_rewrites_alignments_and_names_trees(tmp_path):
    align, out = tmp_path / "aln", tmp_path / "trees"
    align.mkdir()
    (align / "PF00001.aln.masked.faa").write_text(">G1|a*b\nAC*D\n*W\n>G2|c\nAAAA\nAA\n")
    (align / "TIGR00002.v2.aln.masked.faa").write_text(">G1|x\nA*\n")
    (align / "PF00003.other.faa").write_text(">G1|a*\nA*A\n")
    calls = []

    class StandIn(object):
        def infer(self, seqs, model, maxDist):
            calls.append((dict(seqs), model, maxDist))
            return "(%s);" % ",".join(sorted(seqs))

    written = GeneTrees(genomeTree=StandIn()).makeTrees(str(align), str(out), model="poisson", maxDist=2.5)
    assert [os.path.basename(w) for w in written] == ["PF00001.aln.masked.tre", "TIGR00002.v2.aln.masked.tre"]
    assert (align / "PF00001.aln.masked.faa").read_text() == ">G1|a*b\nACXD\nXW\n>G2|c\nAAAA\nAA\n"
    assert (align / "TIGR00002.v2.aln.masked.faa").read_text() == ">G1|x\nAX\n"
    assert (align / "PF00003.other.faa").read_text() == ">G1|a*\nA*A\n"
    assert calls == [({"G1|a*b": "ACXDXW", "G2|c": "AAAAAA"}, "poisson", 2.5), ({"G1|x": "AX"}, "poisson", 2.5)]
    assert (out / "PF00001.aln.masked.tre").read_text() == "(G1|a*b,G2|c);\n"
    assert sorted(os.listdir(str(out))) == ["PF00001.aln.masked.tre", "TIGR00002.v2.aln.masked.tre"]


def test_missing_genome_missing_length_and_non_finite_length_name_the_tree():
    md = synth.metadata(4)
    gt = GeneTrees(runner=emu.runner)
    with pytest.raises(ValueError, match="PF7.tre.*G9"):
        gt.treeTests([("PF7.tre", "(G1|a:0.1,G9|b:0.2);")], md)
    with pytest.raises(ValueError, match="PF8.tre.*without a length"):
        gt.treeTests([("PF8.tre", "(G1|a:0.1,(G2|b,G3|c:0.1):0.2);")], md)
    with pytest.raises(ValueError, match="PF9.tre.*not finite"):
        gt.treeTests([("PF9.tre", "(G1|a:0.1,G2|b:1e999);")], md)
    # the root's own length may be absent or present
    assert gt.treeTests([("ok", "(G1|a:0.1,G2|b:0.2):0.5;")], md)["info"]["python_trees"] == 0


def test_library_refusals():
    md = synth.metadata(8)
    p = geneTrees.packTree("t", "((G1|a:0.1,G1|b:0.2):0.1,(G2|a:0.3,G3|a:0.1):0.2,G1|c:0.0);", md)

    def code(change):
        q = geneTrees.forestTables([p])
        change(q)
        with pytest.raises(_lib.CkmError) as e:
            _lib.genetree_check(q)
        with pytest.raises(_lib.CkmError):
            _lib.genetree_host(q)
        return e.value.code

    _lib.genetree_check(geneTrees.forestTables([p]))
    assert code(lambda q: q.length.__setitem__(2, np.nan)) == -1
    assert code(lambda q: q.length.__setitem__(3, np.inf)) == -1
    assert code(lambda q: q.last.__setitem__(1, 9)) == -1                    # a range outside the tree
    assert code(lambda q: q.parent.__setitem__(2, 5)) == -1                  # a parent behind its child
    assert code(lambda q: q.leaf_class.__setitem__(0, 7)) == -1              # a class index beyond the count
    assert code(lambda q: q.class_total.__setitem__(0, 1)) == -1
    assert code(lambda q: q.pair_b.__setitem__(0, 5)) == -1                  # a pair beyond the tree
    assert code(lambda q: q.pair_b.__setitem__(0, 2)) == -1                  # a pair of two genomes
    many = synth.metadata((1 << 14) + 1, one_class=True)
    big = geneTrees.packTree("big", synth.newick("star", ["G%d|x" % k for k in range((1 << 14) + 1)], random.Random(1)), many)
    with pytest.raises(_lib.CkmError) as e:
        _lib.genetree_check(geneTrees.forestTables([big]))
    assert e.value.code == -7
    deep = geneTrees.packTree("deep", synth.newick("chain", ["G%d|x" % k for k in range(1 << 14)], random.Random(1)), many)
    assert len(deep.first) > (1 << 15)
    with pytest.raises(_lib.CkmError) as e:
        _lib.genetree_check(geneTrees.forestTables([deep]))
    assert e.value.code == -7


def test_python_loop_in_the_library_s_place(monkeypatch):
    trees, md = seeded_forest()
    want = GeneTrees(runner=emu.runner).treeTests(trees, md, geneTrees.genomeIdOfGene)
    # a real tree beyond the limit next to one within it: the star of one class has consistency 1 everywhere
    many = synth.metadata((1 << 14) + 1, one_class=True)
    big = synth.newick("star", ["G%d|x" % k for k in range((1 << 14) + 1)], random.Random(1))
    res = GeneTrees(runner=emu.runner).treeTests([("big", big), trees[0]], dict(md, **many), geneTrees.genomeIdOfGene)
    assert res["info"]["python_trees"] == 1 and res["info"]["ntrees"] == 1
    assert res["consistency"][0].tolist() == [1.0, 1.0, 1.0] and res["pair_flag"][0].size == 0
    # with the limit lowered every tree of more than 20 leaves takes the loop, and nothing changes
    monkeypatch.setattr(_lib, "GENETREE_MAX_LEAVES", 20)
    res = GeneTrees(runner=emu.runner).treeTests(trees, md, geneTrees.genomeIdOfGene)
    assert res["info"]["python_trees"] == sum(len(p.labels) > 20 for p in want["packed"]) > 0
    for f in OUTPUTS:
        for k in range(len(trees)):
            assert res[f][k].tolist() == want[f][k].tolist() and res[f][k].dtype == want[f][k].dtype, (f, k)
