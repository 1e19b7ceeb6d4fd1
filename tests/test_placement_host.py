"""The placement without a device.  The host executor of the kernels' arithmetic (tests/emu/placement: checkm_amd/csrc/place_dev.h under
g++) against a second formulation written independently (tests/emu/placement_oracle: the query inserted in the tree, pruning with numpy,
scipy.linalg.expm for every P(t)): logL to a relative 1e-9 -- every factor is a sum of non-negative products, about 2 x 10^3 operations
at 2^-53 each, plus expm and eigen-route error near 1e-12, two orders below the bound for S <= 4096 -- and the best edge wherever the
oracle's gap between best and second is above 1e-6 |logL|.  The committed recovery fixture (tests/golden/placement_cases.json, made by
tools/gen_placement_golden.py): every pruned leaf goes back on the merged edge it came from, no miss allowed.
_createConcatenatedAlignment against the reference's own output; the tree writer; what ckm_place_check refuses; the level schedule; the
header and the export list."""
import json
import os

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.pplacer import (DEFAULT_DISTAL_FRACTIONS, DEFAULT_PENDANT_GRID, PplacerRunner, RefPkg, discrete_gamma, log_likelihood, nodes_of, parse_newick,
                                read_fasta, read_paml_dat, write_newick)
from checkm_amd.treeParser import TreeParser, read_newick
from tests.emu import placement as emu
from tests.emu import placement_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "placement_cases.json")))
FIELDS = ("top_edge", "scan_m", "scan_e", "ref_m", "ref_e", "ref_f", "ref_g")


def same_bits(a, b):
    for f in FIELDS:
        x, y = a[f], b[f]
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), f


def synthetic(seed, tree_text, nsites, rates=(0.3, 1.7), weights=(0.4, 0.6)):
    """(refpkg, alignment) of a seeded random model with sequences simulated down the tree."""
    rng = np.random.default_rng(seed)
    S, pi = orc.random_model(rng)
    aln = orc.simulate(rng, parse_newick(tree_text), S, pi, rates, weights, nsites)
    return RefPkg(tree_text, aln, S, pi, rates, weights), aln, (S, pi)


def recovery_refpkg(leaf):
    g = GOLDEN["recovery"]
    S = np.zeros((20, 20))
    k = 0
    for i in range(1, 20):
        for j in range(i):
            S[i, j] = S[j, i] = g["exchangeabilities"][k]
            k += 1
    rest = {n: s for n, s in g["alignment"].items() if n != leaf["leaf"]}
    return RefPkg(leaf["tree"], rest, S, np.array(g["frequencies"]), g["rates"], g["weights"])


def check_recovery(place):
    """place(refpkg, queries, pendantGrid, distalFractions) -> placements; every leaf of the fixture back on its edge."""
    g = GOLDEN["recovery"]
    assert len(g["leaves"]) == 16 and len(g["alignment"]["t0"]) == 400 and g["smallest_margin"] >= 1.0
    for leaf in g["leaves"]:
        got = place(recovery_refpkg(leaf), {leaf["leaf"]: g["alignment"][leaf["leaf"]]}, g["pendant"], g["distal"])[leaf["leaf"]]
        assert got[0][0] in leaf["edges"], (leaf["leaf"], got[0], leaf["edges"])
        assert abs(got[0][1] - leaf["oracle_logL"]) <= 1e-9 * abs(leaf["oracle_logL"])


def host_place(refpkg, queries, pendantGrid=None, distalFractions=None, **kw):
    r = PplacerRunner(1)
    t = r._tables(refpkg, queries, pendantGrid, distalFractions, kw.pop("startPend", 0.1), kw.pop("maxPitches", 40))
    return r._placements(t, emu.place_run(None, t, kw.pop("budget_bytes", 0)), **kw)


def test_executor_against_the_brute_force_formulation():
    rng = np.random.default_rng(11)
    text = orc.random_tree(rng, 7, 0.02, 0.6, root_degree=2)
    ref, aln, (S, pi) = synthetic(12, text, 70)
    queries = {"mix": aln["t3"][:35] + "-----" + aln["t4"][40:50].lower() + aln["t4"][50:], "near": aln["t5"][:60] + "XBZJUO*.-a", "gaps": "-" * 70}
    pend, frac = (0.01, 0.1, 1.0), (0.25, 0.75)
    r = PplacerRunner(1)
    t = r._tables(ref, queries, pend, frac, 0.1, 100)
    res = emu.place_run(None, t)
    oracle = orc.Oracle(S, pi, ref.rates, ref.weights)
    nedges = t.nnodes - 1
    assert (res["top_edge"][:, nedges:] == -1).all() and (res["top_edge"][:, :nedges] >= 0).all()
    for qi, name in enumerate(t.names):
        per_edge = {}
        for k in range(nedges):
            e, length = int(res["top_edge"][qi, k]), float(t.length[int(res["top_edge"][qi, k])])
            want = oracle.placed(ref.root, aln, queries[name], e, length / 2, 0.1)
            got = log_likelihood(res["scan_m"][qi, k], int(res["scan_e"][qi, k]))
            assert abs(got - want) <= 1e-9 * abs(want), (name, e, got, want)
            grid = {(fi, gi): oracle.placed(ref.root, aln, queries[name], e, f * length, b) for fi, f in enumerate(frac) for gi, b in enumerate(pend)}
            per_edge[e] = max(grid.values())
            got = log_likelihood(res["ref_m"][qi, k], int(res["ref_e"][qi, k]))
            assert abs(got - per_edge[e]) <= 1e-9 * abs(per_edge[e]), (name, e, got, per_edge[e])
            ranked = sorted(grid.values(), reverse=True)
            if ranked[0] - ranked[1] > 1e-6 * abs(ranked[0]):
                assert grid[(int(res["ref_f"][qi, k]), int(res["ref_g"][qi, k]))] == ranked[0]
        ranked = sorted(per_edge, key=lambda e: -per_edge[e])
        best = r._placements(t, res)[name][0]
        if per_edge[ranked[0]] - per_edge[ranked[1]] > 1e-6 * abs(per_edge[ranked[0]]):
            assert best[0] == ranked[0]
    gaps = t.names.index("gaps")
    assert res["top_edge"][gaps, :nedges].tolist() == list(range(nedges))      # every edge ties bit for bit: the lower edge number first
    assert len(set(res["scan_m"][gaps, :nedges].tolist())) == 1 and not res["ref_f"][gaps, :nedges].any() and not res["ref_g"][gaps, :nedges].any()


def test_recovery_fixture_every_leaf_back_on_its_edge():
    check_recovery(host_place)


def test_no_result_depends_on_the_budget():
    rng = np.random.default_rng(5)
    ref, aln, _ = synthetic(6, orc.random_tree(rng, 5, root_degree=3), 200, rates=(1.0,), weights=(1.0,))
    t = PplacerRunner(1)._tables(ref, {"a": aln["t1"], "b": aln["t2"][:100] + "-" * 100}, (0.05, 0.5), (0.5,), 0.1, 3)
    one = emu.place_run(None, t)
    assert one["nchunks"] == 1 and one["chunk_sites"] == 200
    for budget, chunks in ((1, 4), (130 * emu_site_bytes(t), 2)):
        cut = emu.place_run(None, t, budget)
        assert cut["nchunks"] == chunks
        same_bits(one, cut)


def emu_site_bytes(t):
    return t.nnodes * (2 * t.nrates * 20 * 8 + 8) + t.nnodes * (21 * 8 + 4)


def test_level_schedule():
    rng = np.random.default_rng(3)
    cat = "(a:0.1,b:0.1)"
    for k in range(5):
        cat = "(%s:0.1,c%d:0.1)" % (cat, k)
    ref, aln, _ = synthetic(4, cat + ";", 3, rates=(1.0,), weights=(1.0,))
    up, down = emu.place_levels(PplacerRunner(1)._tables(ref, {"q": "AAA"}))
    assert [len(x) for x in up] == [7, 1, 1, 1, 1, 1, 1] and [len(x) for x in down] == [2] * 6      # a caterpillar: one node per level
    ref, aln, _ = synthetic(4, orc.random_tree(rng, 9, root_degree=3), 3)
    t = PplacerRunner(1)._tables(ref, {"q": "AAA"})
    up, down = emu.place_levels(t)
    assert sorted(sum(up, [])) == list(range(t.nnodes)) and sorted(sum(down, [])) == list(range(t.nnodes - 1)) and len(down[0]) == 3
    seen = set()
    for level in up:                                               # children before parents
        for v in level:
            assert all(int(c) in seen for c in t.child[int(t.child_off[v]):int(t.child_off[v + 1])])
        seen.update(level)


@pytest.mark.parametrize("name", sorted(GOLDEN["concat"]))
def test_concatenated_alignment_against_the_reference(name, tmp_path):
    import types
    case = GOLDEN["concat"][name]
    for marker, seqs in case["files"].items():
        with open(tmp_path / (marker + ".masked.faa"), "w") as f:
            for seq_id, seq in seqs.items():
                f.write(">%s\n%s\n" % (seq_id, seq))
    parser = types.SimpleNamespace(models={"bin": {m: types.SimpleNamespace(leng=n) for m, n in case["lengths"].items()}})
    path = PplacerRunner(1)._createConcatenatedAlignment([], parser, str(tmp_path))
    assert os.path.basename(path) == case["file"] == "concatenated.fasta"
    text = open(path).read()
    assert read_fasta(path) == case["seqs"]
    assert text == "".join(">%s\n%s\n" % (b, case["seqs"][b]) for b in sorted(case["seqs"]))      # the record format; sorted bin order
    if name == "two_markers_one_missing":
        assert case["seqs"]["binB"] == "MRV-LIA" + "-" * 5
    if name == "bin_seen_in_one_marker":
        assert case["seqs"]["y"] == "---" + "DD-D" + "--"


TREE = "((A:0.1,'B c''d':0.2)'U1|k__X|90':0.3,(C:0.1,D:0.4)U2:0.5,E:0.6)'UID1|k__Bacteria|';"


def test_tree_numbering_and_round_trip():
    root = parse_newick(TREE)
    nodes = nodes_of(root)
    assert [v.name for v in nodes] == ["A", "'B c''d'", "'U1|k__X|90'", "C", "D", "U2", "E", "'UID1|k__Bacteria|'"]      # as the nodes close
    assert write_newick(root) == TREE
    jp = write_newick(root, edge_numbers=True)
    assert jp == "((A:0.1{0},'B c''d':0.2{1})'U1|k__X|90':0.3{2},(C:0.1{3},D:0.4{4})U2:0.5{5},E:0.6{6})'UID1|k__Bacteria|';"
    assert write_newick(parse_newick(jp)) == TREE


def test_tree_writer_has_tog_semantics():
    root = parse_newick(TREE)
    ref = type("R", (), {"root": root})
    placements = {"bin2": [(1, -10.0, 1.0, 0.15, 0.07)], "bin1": [(1, -11.0, 1.0, 0.05, 0.01)], "bin0": [(1, -9.0, 1.0, 0.05, 0.02)],      # three on one edge
                  "top bin": [(6, -5.0, 0.9, 0.25, 0.3), (2, -8.0, 0.1, 0.0, 0.1)], "unplaced": []}                                        # a root edge, a quoted name
    text = PplacerRunner.tog(ref, placements)
    assert text == ("((A:0.1,((('B c''d':0.05,bin0:0.02):0.0,bin1:0.01):0.09999999999999999,bin2:0.07):0.05000000000000002)'U1|k__X|90':0.3,"
                    "(C:0.1,D:0.4)U2:0.5,(E:0.25,'top bin':0.3):0.35)'UID1|k__Bacteria|';")
    tree = read_newick(text)                                       # this package's own reader
    assert sorted(leaf.taxon for leaf in tree.root.leaves()) == ["A", "B c'd", "C", "D", "E", "bin0", "bin1", "bin2", "top bin"]
    first = lambda b: TreeParser._first_labelled_ancestor(tree.find_leaf(b)).label
    assert [first(b) for b in ("bin0", "bin1", "bin2")] == ["U1|k__X|90"] * 3 and first("top bin") == "UID1|k__Bacteria|" and tree.find_leaf("unplaced") is None
    b = tree.find_leaf("B c'd")
    assert abs(b.length + b.parent.length + b.parent.parent.length + b.parent.parent.parent.length - 0.2) < 1e-15      # l - d stays above
    assert [c.label for c in tree.root.children if c.label] == ["U1|k__X|90", "U2"] and tree.root.label == "UID1|k__Bacteria|"


def small_tables(**over):
    """A valid call of three leaves on a trifurcating root, with single fields overridden."""
    R, F, G = over.pop("R", 1), 2, 2
    base = dict(child_off=[0, 0, 0, 0, 3], child=[0, 1, 2], length=[0.1, 0.2, 0.3, 0.0], nsites=4, row_off=[0, 4, 8, 12], rows=b"ACDEACDFACDG", q_off=[0, 4], queries=b"AC-E",
                weights=np.full(R, 1.0 / R), U=np.eye(20), Uinv=np.eye(20), pi=np.full(20, 0.05), exp_len=np.ones((4, R, 20)), exp_half=np.ones((4, R, 20)),
                exp_dist=np.ones((4, F, 2, R, 20)), exp_pend=np.ones((1 + G, R, 20)), max_pitches=2)
    base.update(over)
    return _lib.PlaceTables(**base)


def refused(tables):
    with pytest.raises(_lib.CkmError) as e:
        _lib.place_check(tables)
    with pytest.raises(_lib.CkmError) as h:
        emu.place_check(tables)
    assert e.value.code == h.value.code
    return e.value.code


def test_refusals():
    _lib.place_check(small_tables())
    emu.place_check(small_tables())
    assert refused(small_tables(length=[0.1, -0.2, 0.3, 0.0])) == -1
    assert refused(small_tables(length=[0.1, float("nan"), 0.3, 0.0])) == -1
    assert refused(small_tables(length=[float("inf"), 0.2, 0.3, 0.0])) == -1
    assert refused(small_tables(row_off=[0, 4, 9, 12])) == -1                           # a row of five and a row of three
    assert refused(small_tables(row_off=[0, 4, 8, 13])) == -1                           # beyond the bytes
    assert refused(small_tables(q_off=[0, 3], queries=b"ACD")) == -1
    assert refused(small_tables(child=[0, 1, 1])) == -1                                 # a child listed twice
    assert refused(small_tables(child=[0, 1, 3])) == -1                                 # a node as its own child
    assert refused(small_tables(child_off=[0, 0, 0, 2, 3], child=[0, 1, 2])) == -1      # offsets out of order for a tree: node 3 with one child
    assert refused(small_tables(child_off=[0, 0, 3, 2, 3])) == -1                       # offsets that fall
    assert refused(small_tables(child_off=[0, 0, 0, 0, 4])) == -1                       # beyond the children
    assert refused(small_tables(R=9)) == -7                                             # more than 8 rates
    assert refused(small_tables(max_pitches=0)) == -1
    assert refused(small_tables(exp_len=np.full((4, 1, 20), np.nan))) == -1
    _lib.place_check(small_tables(R=8))


def test_models_and_rates(tmp_path):
    rates, weights = discrete_gamma(0.5, 4)
    assert abs(float((rates * weights).sum()) - 1.0) < 1e-12 and (np.diff(rates) > 0).all() and weights.tolist() == [0.25] * 4
    assert np.allclose(rates, [0.03338775, 0.25191592, 0.82026848, 2.89442785], atol=1e-6)      # Yang 1994, alpha = 0.5, four categories
    assert np.allclose(discrete_gamma(1e3, 3)[0], 1.0, atol=0.05)
    rng = np.random.default_rng(1)
    S, pi = orc.random_model(rng)
    with open(tmp_path / "m.dat", "w") as f:
        for i in range(1, 20):
            f.write(" ".join(repr(float(S[i, j])) for j in range(i)) + "\n")
        f.write("\n" + " ".join(repr(float(x)) for x in pi) + "\n\nA R N D ... the prose of a PAML file 1.5 2.5\n")
    S2, pi2 = read_paml_dat(str(tmp_path / "m.dat"))
    assert np.array_equal(S2, S) and np.allclose(pi2, pi, rtol=1e-15)
    ref = RefPkg("(a:0.1,b:0.2,c:0.3);", {"a": "A", "b": "C", "c": "D"}, S, pi)
    from scipy.linalg import expm
    assert np.allclose((ref.U * np.exp(ref.lam * 0.7)[None, :]) @ ref.Uinv, expm(orc.rate_matrix(S, pi) * 0.7), atol=1e-13)
    assert len(DEFAULT_PENDANT_GRID) == 16 and abs(DEFAULT_PENDANT_GRID[0] - 1e-3) < 1e-18 and abs(DEFAULT_PENDANT_GRID[-1] - 2.0) < 1e-12
    assert DEFAULT_DISTAL_FRACTIONS == tuple((2 * k + 1) / 16 for k in range(8))


def test_header_and_exports_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    for n in ("ckm_place_check", "ckm_place_run"):
        assert n + "(" in header and n in _lib.EXPORTS and hasattr(_lib.load(), n)
    assert "#define CKM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.load().ckm_abi_version() == 12
    for line in ("checkm/pplacer.py:70-80", "CKM_PLACE_BATCH_MB", "ckm_place_args;", "ckm_place_out;", "ckm_place_info;"):
        assert line in header
    makefile = open(os.path.join(ROOT, "checkm_amd", "csrc", "Makefile")).read()
    for n in ("place_host.o", "kernels_place.o", "ckm_place.o", "place_dev.h"):
        assert n in makefile


# ---- PplacerRunner.run on a small tree directory, then this package's own TreeParser ----------------------------------------------------
from tests.test_tree_parser import _Results, world      # noqa: E402,F401  (the data directory and the output directory with four bins)

REF_TREE = ("((((IMG_1:0.1,IMG_2:0.1)'UID10|g__A|100':0.1,IMG_3:0.15)'UID5|f__F|90':0.1,IMG_4:0.1)'UID2|k__Bacteria|100':0.3,"
            "(IMG_5:0.2,IMG_6:0.2)'UID3|k__Archaea|100':0.3)'UID1||';")


def run_on_the_tree_directory(out):
    """run() twice in the output directory of tests/test_tree_parser.py's `world`: no *.masked.faa (the reference tree is copied), then
    two markers with binA a copy of IMG_3 and binB a copy of IMG_5 in one marker only.  Returns the lineage marker file's lines."""
    import types
    from checkm_amd.defaultValues import DefaultValues
    ref, aln, (S, pi) = synthetic(21, REF_TREE, 60, rates=(0.5, 1.5), weights=(0.5, 0.5))
    pkg = DefaultValues.PPLACER_REF_PACKAGE_REDUCED
    os.makedirs(pkg)
    json.dump({"files": {"tree": "tree.nwk", "aln_fasta": "ref.fasta"}}, open(os.path.join(pkg, "CONTENTS.json"), "w"))
    open(os.path.join(pkg, "tree.nwk"), "w").write(REF_TREE + "\n")
    open(os.path.join(pkg, DefaultValues.GENOME_TREE), "w").write(REF_TREE + "\n")
    open(os.path.join(pkg, "ref.fasta"), "w").write("".join(">%s\n%s\n" % kv for kv in sorted(aln.items())))
    model = os.path.join(pkg, "model.dat")
    with open(model, "w") as f:
        for i in range(1, 20):
            f.write(" ".join(repr(float(S[i, j])) for j in range(i)) + "\n")
        f.write("\n" + " ".join(repr(float(x)) for x in pi) + "\n")
    parser = types.SimpleNamespace(models={"binA": {"M1": types.SimpleNamespace(leng=30), "M2": types.SimpleNamespace(leng=30)}})
    tree_dir = os.path.join(out, "storage", "tree")
    os.remove(os.path.join(tree_dir, "concatenated.tre"))
    runner = PplacerRunner(1, modelFile=model, rates=(0.5, 1.5), weights=(0.5, 0.5))
    runner.run(["binA", "binB"], parser, out, True)
    assert open(os.path.join(tree_dir, "concatenated.tre")).read() == REF_TREE + "\n" and os.path.getsize(os.path.join(tree_dir, "concatenated.fasta")) == 0
    assert not os.path.exists(os.path.join(tree_dir, "concatenated.pplacer.json"))
    open(os.path.join(tree_dir, "M1.masked.faa"), "w").write(">binA&&g1\n%s\n>binB&&g7\n%s\n" % (aln["IMG_3"][:30], aln["IMG_5"][:30]))
    open(os.path.join(tree_dir, "M2.masked.faa"), "w").write(">binA&&g2\n%s\n" % aln["IMG_3"][30:])
    runner.run(["binA", "binB"], parser, out, True)
    assert read_fasta(os.path.join(tree_dir, "concatenated.fasta")) == {"binA": aln["IMG_3"], "binB": aln["IMG_5"][:30] + "-" * 30}
    jp = json.load(open(os.path.join(tree_dir, "concatenated.pplacer.json")))
    assert jp["version"] == 3 and jp["fields"] == ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]
    assert "{0}" in jp["tree"] and write_newick(parse_newick(jp["tree"])) == REF_TREE and [p["n"] for p in jp["placements"]] == [["binA"], ["binB"]]
    for p in jp["placements"]:
        assert 1 <= len(p["p"]) <= 7 and abs(sum(r[2] for r in p["p"]) - 1.0) < 0.05 and all(r[2] >= 0.01 * p["p"][0][2] for r in p["p"])
    nodes = nodes_of(parse_newick(REF_TREE))
    assert nodes[jp["placements"][0]["p"][0][0]].name == "IMG_3" and nodes[jp["placements"][1]["p"][0][0]].name == "IMG_5"
    assert open(os.path.join(tree_dir, "pplacer.out")).read().startswith("checkm_amd placement: 2 queries, 10 edges, 60 sites, 2 rate categories\n")
    tp = TreeParser()
    assert tp.getInsertionBranchId(out, ["binA", "binB", "binC"]) == {"binA": "UID5", "binB": "UID3", "binC": "NA"}
    path = os.path.join(out, "lineage.ms")
    tp.getBinMarkerSets(out, path, 30, 0, True, False, False, _Results(binA=(40, 0), binB=(40, 0), binC=(40, 0), binD=(40, 0)), 10, 10)
    return open(path).read().splitlines()


def test_run_then_tree_parser_with_the_host_executor(world, monkeypatch):      # noqa: F811
    from checkm_amd import runtime
    monkeypatch.setattr(_lib, "place_run", emu.place_run)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    lines = run_on_the_tree_directory(world)
    check_lineage_lines(lines)


def check_lineage_lines(lines):
    rows = {ln.split("\t")[0]: ln.split("\t") for ln in lines[1:]}
    assert lines[0] == "# [Lineage Marker File]" and sorted(rows) == ["binA", "binB", "binC", "binD"]
    assert rows["binA"][2::4] == ["UID5", "UID2", "UID1"] and rows["binB"][2::4] == ["UID3", "UID1"] and rows["binC"][2::4] == ["UID1"] == rows["binD"][2::4]
