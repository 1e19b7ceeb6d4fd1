"""The scaffold simulation without a device: every golden case (tests/golden/simscaffolds_cases.json, made by
tools/gen_simscaffolds_golden.py from the reference's own img.py, markerSetBuilder.py, the two simulationScaffolds scripts and
checkm.markerSets) through markerGenesOnScaffolds, through scaffoldChecks on the host executor of the kernel's arithmetic
(tests/emu/simscaf) and through checkm_amd.simulationScaffolds.SimulationScaffolds with the executor in the device's place, all at ==,
the two texts byte for byte, the draws from the seeds; the tree walk and buildBinMarkerSetsLOO against the reference's chains; the IMG
additions; the executor against the plain loop on a seeded synthetic case; what the library refuses; the header and the export list."""
from collections import defaultdict
import gzip
import json
import os
import random
import warnings

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd.img import IMG
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from checkm_amd.markerSets import BinMarkerSets, MarkerSet
from checkm_amd.simulationScaffolds import SimulationScaffolds
from checkm_amd.treeParser import read_newick
from tests.emu import markerset as mset_emu
from tests.emu import simscaf as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "simscaffolds_cases.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}
MODES = ("inv_length", "random")


def use_host_executor(monkeypatch):
    """The device entry of checkm_amd._lib replaced by the host executor; ckm_simscaf_check stays the library's (it needs no device)."""
    monkeypatch.setattr(_lib, "simscaf_run", emu.simscaf_run)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)


def write_tree(d, c):
    files = dict(c["files"])
    for g, src in c["same_as"].items():
        files.update(("%s/%s%s" % (g, g, rel[len(src) * 2 + 1:]), text) for rel, text in c["files"].items() if rel.startswith(src + "/"))
    for rel, text in files.items():
        p = os.path.join(str(d), *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    open(os.path.join(str(d), "tigrfam2pfam.tsv"), "w").write(c["redundant"])
    return sorted(set(rel.split("/")[0] for rel in files))


def builder_of(d, c):
    """A MarkerSetBuilder over the case's genome directory, the scaffold and length caches made."""
    ids = write_tree(d, c)
    b = MarkerSetBuilder(IMG(None, os.path.join(str(d), "tigrfam2pfam.tsv"), str(d)))
    b.precomputeGenomeFamilyScaffolds(ids)
    b.precomputeGenomeSeqLens(ids)
    return b


def marker_sets(rows):
    return [MarkerSet(s["UID"], s["lineageStr"], s["numGenomes"], [set(x) for x in s["sets"]]) for s in rows]


def bin_marker_sets(binId, rows):
    b = BinMarkerSets(binId, BinMarkerSets.TREE_MARKER_SET)
    for ms in marker_sets(rows):
        b.addMarkerSet(ms)
    return b


def draws_of(run):
    return [(d["retained"], d["contGenomeId"], d["contSampled"]) for d in run["draws"]]


def wanted_checks(run):
    return [[[float.fromhex(v) for v in row] for row in d["checks"]] for d in run["draws"]]


def check_case(b, c, mode):
    """The golden's draws through markerGenesOnScaffolds, the plain genomeCheck and scaffoldChecks (one call for all draws), and the
    whole case through SimulationScaffolds.evaluate.  runtime.get_ctx and _lib.simscaf_run are whatever the caller installed."""
    run = c["runs"][mode]
    sets, want = marker_sets(c["chain"] + c["refined"]), wanted_checks(run)
    for d, w in zip(run["draws"], want):
        for s, ms in enumerate(sets):
            contained = defaultdict(list)
            b.markerGenesOnScaffolds(ms.getMarkerGenes(), c["genomeId"], d["retained"], contained)
            b.markerGenesOnScaffolds(ms.getMarkerGenes(), d["contGenomeId"], d["contSampled"], contained)
            assert {m: sorted(v) for m, v in contained.items()} == d["contained"][s]
            assert list(b._genome_check_host(ms, contained)) == w[s]
    got = b.scaffoldChecks(sets, c["genomeId"], draws_of(run))
    assert b.last_scaffold_timing["device"] and got.shape == (len(run["draws"]), len(sets), 4) and got.tolist() == want
    sim = SimulationScaffolds(b, mode, c["contigLens"], c["percentComps"], c["percentConts"])
    random.seed(c["seed"]); np.random.seed(c["seed"])
    results = sim.evaluate(c["genomeId"], bin_marker_sets(c["genomeId"], c["chain"]), bin_marker_sets(c["genomeId"], c["refined"]), c["candidates"], c["numReplicates"],
                           c["taxonomy"])
    assert b.last_scaffold_timing["device"]
    assert [(list(d[0]), d[1], list(d[2]), d[3], d[4]) for d in sim.last_draws] == \
        [(d["retained"], d["contGenomeId"], d["contSampled"], d["trueComp"], d["trueCont"]) for d in run["draws"]]          # the draws from the seeds
    assert json.loads(json.dumps(results)) == run["tuples"] and all(len(t) == 18 for t in results)
    return sim, results


def test_golden_holds_what_the_issue_asks():
    assert sorted(CASES) == ["copies", "thirds_and_sevenths"] and all(sorted(c["runs"]) == list(MODES) for c in CASES.values())
    c = CASES["copies"]
    table = c["img"]["T"]["cluster_scaffold"]
    assert len(c["img"]["T"]["seq_ids"]) == 12 and len(c["candidates"]) - 1 == 2
    assert {len(table.get(m, [])) for ms in c["chain"] for cs in ms["sets"] for m in cs} == {0, 1, 2, 5}
    assert table["pfam10002"][0] == table["pfam10002"][1]                                                  # two copies on one scaffold
    assert table["pfam10006"] == ["ghost"] and "ghost" not in c["img"]["T"]["seq_ids"]                    # a copy on a scaffold the FASTA lacks
    assert "pfam10000" not in table and all("pfam10000" in c["img"][g]["cluster_scaffold"] for g in ("C1", "C2"))
    assert sum("pfam10007" in s for s in c["chain"][0]["sets"]) == 2
    assert c["chain"][1]["lineageStr"] == c["chain"][2]["lineageStr"] not in [s["lineageStr"] for s in c["refined"]]
    assert 0.0 in c["percentConts"] and 0.2 in c["percentConts"] and 0.5 in c["percentComps"] and 1.0 in c["percentComps"] and len(c["contigLens"]) > 1
    for mode in MODES:
        counts = set(len(v) for d in c["runs"][mode]["draws"] for s in d["contained"] for v in s.values())
        assert {1, 2} <= counts and "\tnan\tnan" in c["runs"][mode]["summary"]
        assert len(set(d["contGenomeId"] for d in c["runs"][mode]["draws"])) == 2
    # the by-length script adds a contaminant scaffold at contamination 0.0, the random script none
    assert all(d["contSampled"] for d in c["runs"]["inv_length"]["draws"]) and any(not d["contSampled"] for d in c["runs"]["random"]["draws"] if d["percentCont"] == 0.0)
    assert set(len(s) for s in CASES["thirds_and_sevenths"]["chain"][0]["sets"]) == {3, 7}
    kinds = set((w["bMarkerSet"], w["domain"], w["root_named"]) for w in GOLDEN["walk"]["chains"])
    assert len(kinds) == 8 and "contaminant sampled from the sorted candidates" in GOLDEN["substitutions"]["scripts"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_on_the_host_executor(name, mode, monkeypatch, tmp_path):
    use_host_executor(monkeypatch)
    c = CASES[name]
    sim, results = check_case(builder_of(tmp_path / "genomes", c), c, mode)
    summary, replicates = str(tmp_path / "summary.tsv"), str(tmp_path / "replicates.tsv.gz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                              # numpy's mean of an empty list: the reference's nan columns
        sim.write(results, summary, replicates)
        assert open(summary, "rb").read() == c["runs"][mode]["summary"].encode() and gzip.open(replicates, "rb").read() == c["runs"][mode]["replicates"].encode()


def test_sequence_lengths_come_from_the_cache(monkeypatch, tmp_path):
    use_host_executor(monkeypatch)
    c = CASES["copies"]
    b = builder_of(tmp_path, c)

    def never(genomeId):
        raise AssertionError("a FASTA file was read again")
    monkeypatch.setattr(b.img, "_genomeSeqLens", never)
    calls = []
    inner = b.scaffoldChecks
    monkeypatch.setattr(b, "scaffoldChecks", lambda *a: calls.append(1) or inner(*a))
    check = SimulationScaffolds(b, "random", c["contigLens"], c["percentComps"], c["percentConts"])
    check.evaluate(c["genomeId"], bin_marker_sets("T", c["chain"]), bin_marker_sets("T", c["refined"]), c["candidates"], 2, c["taxonomy"])
    assert calls == [1]                                                               # all draws of the genome in one call
    with pytest.raises(ValueError):
        SimulationScaffolds(b, "by_length")


def test_img_additions(tmp_path):
    for c in CASES.values():
        ids = write_tree(tmp_path / c["name"], c)
        img = IMG(None, None, str(tmp_path / c["name"]))
        for g in ids:
            want = c["img"][g]
            assert {f: sorted(v) for f, v in img._genomeIdToClusterScaffold(g).items()} == want["cluster_scaffold"]
            assert list(img._genomeSeqLens(g).keys()) == want["seq_ids"]
            if "gene_scaffold" in want:
                assert img.geneIdToScaffoldId(g) == want["gene_scaffold"]
        assert img.precomputeGenomeFamilyScaffolds(ids) is img.cachedGenomeFamilyScaffolds and sorted(img.cachedGenomeFamilyScaffolds) == ids
        f = c["img"]["filter"]
        assert sorted(img.filterGenomeIds(f["genomeIds"], f["metadata"], f["field"], f["value"])) == f["kept"]
    img = IMG(None, None, str(tmp_path / "copies"))
    assert "tnogff" not in img.geneIdToScaffoldId("T") and len(img._genomeIdToClusterScaffold("T")["pfam10008"]) == 1      # a gene without a GFF record is dropped
    assert len(img.geneIdToScaffoldId("C1")) == 5                                     # the eight-field line is skipped


# ---- the tree walk ----------------------------------------------------------------------------------------------------------------------------
def walk_builder(d, root_named, monkeypatch):
    """A MarkerSetBuilder over the walk's genome directory with its three data files read from disk, the marker and co-location passes on
    the host executor of tests/emu/markerset."""
    w = GOLDEN["walk"]
    write_tree(d, w)
    for name, key in (("metadata.tsv", "metadata_named" if root_named else "metadata_root_unnamed"), ("derep.txt", "derep"), ("missing_duplicate.tsv", "missing_duplicate")):
        open(os.path.join(str(d), name), "w").write(w[key])
    b = MarkerSetBuilder(IMG(None, os.path.join(str(d), "tigrfam2pfam.tsv"), str(d)))
    stats = b.readNodeMetadata(os.path.join(str(d), "metadata.tsv"))
    assert stats["UID6"]["bootstrap"] == "NA" and stats["UID3"]["taxonomy"] == "k__Bacteria;p__P" and stats["UID4"]["taxonomy"] == ""
    assert b.readDuplicateSeqs(os.path.join(str(d), "derep.txt")) == {"IMG_W3": ["IMG_W7"]}
    assert b.readLineageSpecificGenesToRemove(os.path.join(str(d), "missing_duplicate.tsv"))["UID5"] == {"pfam30003", "pfam30002"}
    for n in ("MsetTable", "mset_markers", "mset_colocated"):
        monkeypatch.setattr(_lib, n, getattr(mset_emu, n))
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    return b


def sets_of(binMarkerSets):
    return [dict(lineageStr=ms.lineageStr, numGenomes=ms.numGenomes, UID=ms.UID, sets=sorted(sorted(s) for s in ms.markerSet)) for ms in binMarkerSets.markerSetIter()]


@pytest.mark.parametrize("root_named", [True, False])
def test_tree_walk_against_the_reference(root_named, monkeypatch, tmp_path):
    w = GOLDEN["walk"]
    b = walk_builder(tmp_path, root_named, monkeypatch)
    tree = read_newick(w["newick"])
    seen = 0
    for g in w["chains"]:
        if g["root_named"] != root_named:
            continue
        node = tree.find_leaf("IMG_" + g["genomeId"]).parent
        build = b.buildDomainMarkerSet if g["domain"] else b.buildBinMarkerSet
        chain, refined = build(tree, node, w["ubiquity"], w["single"], bMarkerSet=g["bMarkerSet"], genomeIdsToRemove=[g["genomeId"]])
        assert chain.binId == refined.binId == g["binId"] and sets_of(chain) == g["chain"] and sets_of(refined) == g["refined"], g
        seen += 1
    assert seen == 16
    rows = [g for g in w["chains"] if g["root_named"] == root_named and not g["domain"] and g["bMarkerSet"]]
    w1 = [g for g in rows if g["genomeId"] == "W1"][0]
    assert [s["lineageStr"] for s in w1["chain"]][0] == "UID4 | p__P" and w1["chain"][0]["numGenomes"] == 4          # UID5 kept one genome; the duplicate W7 counts
    assert w1["chain"][-1]["lineageStr"] == ("UID2 | k__Bacteria" if root_named else "UID2 | root")
    assert any(g["chain"] != g["refined"] for g in rows) and len(set(json.dumps(g["chain"]) for g in rows)) == len(rows)


@pytest.mark.parametrize("bMarkerSet", [True, False])
def test_leave_one_out_chains_from_one_call(bMarkerSet, monkeypatch, tmp_path):
    w = GOLDEN["walk"]
    b = walk_builder(tmp_path, True, monkeypatch)
    tree = read_newick(w["newick"])
    calls = []
    inner = b.buildMarkerSets
    monkeypatch.setattr(b, "buildMarkerSets", lambda lists, *a, **k: calls.append(len(lists)) or inner(lists, *a, **k))
    ids = ["W1", "W2", "W3", "W4", "W5", "W6", "W8"]
    loo = b.buildBinMarkerSetsLOO(tree, ids, w["ubiquity"], w["single"], bMarkerSet=bMarkerSet)
    assert len(calls) == (1 if bMarkerSet else 0)                                    # every (genome, ancestor) list in ONE call
    assert sorted(loo) == ids
    for g in ids:
        chain, refined = b.buildBinMarkerSet(tree, tree.find_leaf("IMG_" + g).parent, w["ubiquity"], w["single"], bMarkerSet=bMarkerSet, genomeIdsToRemove=[g])
        assert sets_of(loo[g][0]) == sets_of(chain) and sets_of(loo[g][1]) == sets_of(refined) and loo[g][0].binId == chain.binId
    for g in w["chains"]:
        if g["root_named"] and not g["domain"] and g["bMarkerSet"] == bMarkerSet:
            assert sets_of(loo[g["genomeId"]][0]) == g["chain"] and sets_of(loo[g["genomeId"]][1]) == g["refined"]


# ---- a seeded synthetic case ------------------------------------------------------------------------------------------------------------------
class TablesOnly(object):
    """An IMG stand-in that holds the scaffold cache alone."""
    def __init__(self, cachedGenomeFamilyScaffolds):
        self.cachedGenomeFamilyScaffolds = cachedGenomeFamilyScaffolds


def synthetic_case(seed, ngenomes=5, nmarkers=90, nsets=5, ndraws=14, nscaffolds=(1, 31, 33, 64, 70)):
    """(builder, marker sets, test genome, draws): genomes of 1 to 70 scaffolds, copies from none to five with repeats on a scaffold, a
    tenth of the markers absent from a genome, markers in two co-located sets of a marker set; draws that keep none, some and all
    scaffolds, name ids no genome has, repeat an id, have no contaminant, and take the test genome as its own contaminant."""
    rng = random.Random(seed)
    names = ["m%03d" % k for k in range(nmarkers)]
    genomes = ["g%d" % k for k in range(ngenomes)]
    scaf = {g: ["%s_s%d" % (g, k) for k in range(n)] for g, n in zip(genomes, nscaffolds)}
    cached = {g: {m: [rng.choice(scaf[g]) for _ in range(rng.choice([1, 1, 1, 2, 3, 5]))] for m in names if rng.random() > 0.1} for g in genomes}
    sets = []
    for s in range(nsets):
        mine = rng.sample(names, rng.randrange(1, nmarkers))
        cs, at = [], 0
        while at < len(mine):
            n = rng.choice([1, 1, 2, 3, 7])
            cs.append(set(mine[at:at + n]) | (set(rng.sample(mine, 1)) if rng.random() < 0.2 else set()))
            at += n
        sets.append(MarkerSet("UID%d" % s, "lineage%d" % (s % 3), 10 + s, cs))
    test = genomes[-1]
    some = lambda g: [s for s in scaf[g] if rng.random() < 0.5]
    draws = [(some(test), rng.choice(genomes[:-1]), some(rng.choice(genomes[:-1]))) for _ in range(ndraws)]
    draws = [(kept, g, some(g)) for kept, g, _ in draws]
    draws[0] = ([], None, [])
    draws[1] = (list(scaf[test]), genomes[3], list(scaf[genomes[3]]))
    draws[2] = (some(test) + ["unknown", scaf[test][0], scaf[test][0]], genomes[0], ["g0_s0", "nobody"])
    draws[3] = (some(test), test, some(test))
    draws[4] = (some(test), None, ["ignored"])
    draws[5] = (list(scaf[test]), genomes[1], [])
    return MarkerSetBuilder(TablesOnly(cached)), sets, test, draws


def test_host_executor_against_the_plain_loop(monkeypatch):
    use_host_executor(monkeypatch)
    b, sets, test, draws = synthetic_case(3)
    want = b._scaffold_checks_host(sets, test, draws)
    got = b.scaffoldChecks(sets, test, draws)
    assert b.last_scaffold_timing["device"] and b.last_scaffold_timing["rounds"] == 1 and np.array_equal(got, want)
    assert len(set(want[:, :, 1].reshape(-1).tolist())) > 10 and want[0].tolist() == [[0.0] * 4] * len(sets) and want[:, :, 1].max() > 0
    tables = b._scaffold_tables(sets, test, draws)
    assert tables.cont[0] == _lib.SIMSCAF_NONE and tables.cont[3] == 0 and tables.ngenomes == 5
    for budget, rounds in ((1, len(draws)), (700, None), (1 << 30, 1)):
        r = emu.simscaf_run(None, tables, budget_bytes=budget)
        assert np.array_equal(r["out"], want) and (rounds is None or r["nrounds"] == rounds) and r["nrounds"] >= 1, budget
    assert 1 < emu.simscaf_run(None, tables, budget_bytes=700)["nrounds"] < len(draws)
    assert b.scaffoldChecks(sets, test, []).shape == (0, len(sets), 4)
    assert b.scaffoldChecks([], test, draws).shape == (len(draws), 0, 4)


def small_tables(**changes):
    """Two genomes of 33 and 3 scaffolds, three markers, two marker sets, three replicates (a contaminant, none, the test genome itself)."""
    t = dict(nscaf=[33, 3], nmarkers=3, sc_off=[0, 1, 3, 3, 4, 4, 6], sc=[32, 0, 0, 2, 1, 1], ms_off=[0, 2, 3], cs_off=[0, 2, 3, 5], cs_marker=[0, 1, 2, 1, 0],
             test=[0, 1, 0], cont=[1, _lib.SIMSCAF_NONE, 0], bit_off=[0, 3, 4, 8], bits=[1, 1, 5, 7, 0xffffffff, 1, 0, 0])
    t.update(changes)
    return _lib.SimScafTables(**t)


def test_refusals():
    _lib.simscaf_check(small_tables())
    emu.simscaf_check(small_tables())
    out = emu.simscaf_run(None, small_tables())["out"]
    assert out.shape == (3, 2, 4) and out[0, 0].tolist() == [100 * 2.0 / 3, 100 * 2.0 / 3, 50.0, 50.0]

    def refused(code, **changes):
        for check in (_lib.simscaf_check, emu.simscaf_check):
            with pytest.raises(_lib.CkmError) as e:
                check(small_tables(**changes))
            assert e.value.code == code, (check, changes)
    refused(-1, sc_off=[1, 1, 3, 3, 4, 4, 6])
    refused(-1, sc_off=[0, 2, 1, 3, 4, 4, 6])                      # falls
    refused(-1, sc_off=[0, 1, 3, 3, 4, 4, 7])                      # beyond the copies
    refused(-1, sc=[33, 0, 0, 2, 1, 1])                            # a scaffold index beyond the test genome's scaffolds
    refused(-1, sc=[32, 0, 0, 3, 1, 1])                            # ... beyond the second genome's
    refused(-1, test=[0, 2, 0], bit_off=[0, 3, 4, 8])              # a genome index beyond the genomes
    refused(-1, cont=[2, _lib.SIMSCAF_NONE, 0])
    refused(-1, bit_off=[0, 2, 4, 8])                              # a bit row of the wrong length
    refused(-1, bit_off=[0, 3, 5, 8])                              # a row for a contaminant that is NONE
    refused(-1, bit_off=[0, 3, 4, 9])                              # beyond the bits
    refused(-1, bit_off=[0, 3, 2, 8])
    refused(-1, bit_off=[1, 3, 4, 8])
    refused(-1, bits=[1, 2, 5, 7, 0xffffffff, 1, 0, 0])            # bit 33 of a genome of 33 scaffolds
    refused(-1, bits=[1, 1, 8, 7, 0xffffffff, 1, 0, 0])            # bit 3 of a genome of 3 scaffolds
    refused(-1, bits=[1, 1, 5, 7, 0xffffffff, 1, 0, 2])            # the same in a contaminant that is the test genome
    refused(-1, ms_off=[0, 2, 4])                                  # beyond the co-located sets
    refused(-1, cs_off=[0, 2, 3, 6])                               # beyond the members
    refused(-1, cs_marker=[0, 1, 3, 1, 0])                         # a marker beyond the markers
    refused(-1, cs_off=[0, 2, 2, 5])                               # a co-located set of size 0
    refused(-1, ms_off=[0, 3, 3])                                  # a marker set with no sets
    refused(-7, nscaf=[33, 2**30 + 1])                             # sizes beyond the limits
    with pytest.raises(_lib.CkmError):
        emu.simscaf_run(None, small_tables(ms_off=[0, 3, 3]))
    with pytest.raises(ValueError):
        small_tables(test=[0, 1])
    with pytest.raises(ValueError):
        small_tables(sc_off=[0, 1, 3, 3, 4, 4])


def test_refused_calls_take_the_plain_loop(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(_lib, "simscaf_run", never)
    monkeypatch.setattr(runtime, "get_ctx", never)
    b = MarkerSetBuilder(TablesOnly({"t": {"A": ["s1"], "B": ["s1", "s2"]}, "c": {"A": ["x"]}}))
    ms = MarkerSet("U", "L", 3, [{"A", "B"}, {"C"}])
    for broken in (MarkerSet("U", "L", 3, []), MarkerSet("U", "L", 3, [{"A"}, set()])):
        with pytest.raises(ZeroDivisionError):                     # the reference's own failure, before any launch
            b.scaffoldChecks([ms, broken], "t", [(["s1"], "c", ["x"])])
        assert not b.last_scaffold_timing["device"]
    assert b._scaffold_checks_host([ms], "t", [(["s1", "s2"], "c", ["x"])]).tolist() == [[[100 * 2.0 / 3, 100 * 2.0 / 3, 50.0, 50.0]]]


def test_without_a_device_the_device_method_raises():
    b = MarkerSetBuilder(TablesOnly({"t": {"A": ["s1"]}}))
    call = ([MarkerSet("U", "L", 3, [{"A"}])], "t", [(["s1"], None, [])])
    if _lib.device_count() > 0:
        assert b.scaffoldChecks(*call).tolist() == [[[100.0, 0.0, 100.0, 0.0]]] and b.last_scaffold_timing["device"]
        return
    with pytest.raises(_lib.CkmError) as e:
        b.scaffoldChecks(*call)
    assert e.value.code == _lib.ENODEV


def test_header_and_exports_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    for n in ("ckm_simscaf_check", "ckm_simscaf_run"):
        assert n + "(" in header and n in _lib.EXPORTS and hasattr(_lib.load(), n)
    assert "#define CKM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.load().ckm_abi_version() == 12
    for line in ("scripts/simulationScaffoldsRandom.py", "scripts/simulationScaffoldsByLength.py", ":371-378", "CKM_SIMSCAF_BATCH_MB", "ckm_simscaf_args;", "CKM_SIMSCAF_NONE"):
        assert line in header
    makefile = open(os.path.join(ROOT, "checkm_amd", "csrc", "Makefile")).read()
    for n in ("simscaf_host.o", "kernels_simscaf.o", "ckm_simscaf.o", "simscaf_dev.h", "sim_score.h"):
        assert n in makefile
    assert "marker_sets.h" in makefile
    for header in ("simscaf_dev.h", "select_dev.h"):
        dev = open(os.path.join(ROOT, "checkm_amd", "csrc", header)).read()
        assert '#include "marker_sets.h"' in dev and "msets::pack(" in dev and "msets::check_marker_sets(" in dev
        for restated in ("void set_terms(", "void finish(", "REPEAT"):       # marker_sets.h's, used and not restated (REPEAT: the repeat marking)
            assert restated not in dev
