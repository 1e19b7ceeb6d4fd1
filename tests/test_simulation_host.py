"""The marker-set simulation without a device: every golden case (tests/golden/simulation_cases.json, made by tools/gen_simulation_golden.py
from the reference's own markerSetBuilder.py, simulation.py and checkm.markerSets) through the host methods of
checkm_amd.markerSetBuilder.MarkerSetBuilder (the draws from the seed), through the host executor of the kernel's arithmetic
(tests/emu/simulation) and through checkm_amd.simulation.Simulation with the executor in the device's place, all at ==, the two texts
byte for byte; the executor against containedMarkerGenes + genomeCheck on a seeded synthetic case; what the library refuses; the header
and the export list."""
import gzip
import json
import os
import random
import warnings

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from checkm_amd.markerSets import BinMarkerSets, MarkerSet
from checkm_amd.simulation import Simulation
from tests.emu import simulation as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "simulation_cases.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def use_host_executor(monkeypatch):
    """The device entry of checkm_amd._lib replaced by the host executor; ckm_sim_check stays the library's (it needs no device)."""
    monkeypatch.setattr(_lib, "sim_run", emu.sim_run)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)


def marker_sets(rows):
    return [MarkerSet(s["UID"], s["lineageStr"], s["numGenomes"], [set(x) for x in s["sets"]]) for s in rows]


def bin_marker_sets(binId, rows):
    b = BinMarkerSets(binId, BinMarkerSets.TREE_MARKER_SET)
    for ms in marker_sets(rows):
        b.addMarkerSet(ms)
    return b


def wanted_checks(c):
    return [[[float.fromhex(v) for v in row] for row in d["checks"]] for d in c["draws"]]


def check_draws_from_the_seed(c):
    """sampleGenome over the case's grid, in the reference's loop order, after seeding both generators as the golden's run did."""
    b = MarkerSetBuilder(None)
    random.seed(c["seed"]); np.random.seed(c["seed"])
    sampled = [d for d in c["draws"] if not d.get("explicit")]
    k = 0
    for contigLen in c["contigLens"]:
        for percentComp in c["percentComps"]:
            for percentCont in c["percentConts"]:
                for _ in range(c["numReplicates"]):
                    trueComp, trueCont, starts = b.sampleGenome(c["genomeSize"], percentComp, percentCont, contigLen)
                    d = sampled[k]; k += 1
                    assert (trueComp, trueCont, starts) == (d["trueComp"], d["trueCont"], d["starts"]) and all(type(s) is int for s in starts)
    assert k == len(sampled) > 0


def check_case(c):
    """The golden's draws through containedMarkerGenes, the plain genomeCheck, genomeChecks (one call for all draws), and the whole case
    through Simulation.evaluate and write.  runtime.get_ctx and _lib.sim_run are whatever the caller installed."""
    b = MarkerSetBuilder(None)
    sets, want = marker_sets(c["chain"] + c["refined"]), wanted_checks(c)
    for d, w in zip(c["draws"], want):
        for s, ms in enumerate(sets):
            contained = b.containedMarkerGenes(ms.getMarkerGenes(), c["positions"], d["starts"], d["contigLen"])
            assert contained == d["contained"][s]
            assert list(b._genome_check_host(ms, contained)) == w[s]
    got = b.genomeChecks(sets, c["positions"], [d["starts"] for d in c["draws"]], [d["contigLen"] for d in c["draws"]])
    assert b.last_sim_timing["device"] and got.shape == (len(c["draws"]), len(sets), 4) and got.tolist() == want
    shuffled = [list(reversed(d["starts"])) for d in c["draws"]]                      # the starts need not come sorted
    assert b.genomeChecks(sets, c["positions"], shuffled, [d["contigLen"] for d in c["draws"]]).tolist() == want
    sim = Simulation(b, c["contigLens"], c["percentComps"], c["percentConts"])
    random.seed(c["seed"]); np.random.seed(c["seed"])
    results = sim.evaluate(c["genomeId"], bin_marker_sets(c["genomeId"], c["chain"]), bin_marker_sets(c["genomeId"], c["refined"]), c["positions"], c["genomeSize"],
                           c["numReplicates"], c["taxonomy"])
    assert b.last_sim_timing["device"]
    assert json.loads(json.dumps(results)) == c["tuples"]
    return sim, results


def test_golden_holds_what_the_issue_asks():
    assert sorted(CASES) == ["edges", "thirds_and_sevenths"] and len(GOLDEN["scaffolds"]) == 4
    c = CASES["edges"]
    counts = set(len(v) for d in c["draws"] for s in d["contained"] for v in s.values())
    assert {1, 2, 3} <= counts                                                        # a contig drawn twice, and three times
    assert any(d["starts"] == [] for d in c["draws"]) and 0.0 in c["percentConts"] and 1.0 in c["percentComps"]
    assert set(len(p) for p in c["positions"].values()) == {0, 1, 2, 5}
    assert "M_absent" not in c["positions"] and sum("M_two" in s for s in c["chain"][0]["sets"]) == 2
    assert c["chain"][1]["lineageStr"] == c["chain"][2]["lineageStr"] not in [s["lineageStr"] for s in c["refined"]]
    t = CASES["thirds_and_sevenths"]
    assert len(t["chain"][0]["sets"]) > 64 and set(len(s) for s in t["chain"][0]["sets"]) == {3, 7}


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_draws_from_the_seed(name):
    check_draws_from_the_seed(CASES[name])


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_on_the_host_executor(name, monkeypatch, tmp_path):
    use_host_executor(monkeypatch)
    c = CASES[name]
    sim, results = check_case(c)
    summary, replicates = str(tmp_path / "summary.tsv"), str(tmp_path / "replicates.tsv.gz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                              # numpy's mean of an empty list: the reference's nan columns
        sim.write(results, summary, replicates)
    assert open(summary, "rb").read() == c["summary"].encode() and gzip.open(replicates, "rb").read() == c["replicates"].encode()
    if name == "edges":
        assert "\tnan\tnan" in c["summary"]                                           # the lineage the refined chain lacks


def test_scaffold_sampling_and_uniformity_goldens():
    b = MarkerSetBuilder(None)
    for c in GOLDEN["scaffolds"]:
        np.random.seed(c["seed"])
        ids, per = b.sampleGenomeScaffoldsInvLength(c["targetPer"], c["seqLens"], c["genomeSize"])
        assert [list(ids), per.hex()] == c["inv_length"]
        ids, per = b.sampleGenomeScaffoldsWithoutReplacement(c["targetPer"], c["seqLens"], c["genomeSize"])
        assert [list(ids), per.hex()] == c["without_replacement"]
        for pts, u in c["uniformity"]:
            assert b.uniformity(c["genomeSize"] if len(pts) == 9 else 40 if len(pts) == 4 else 100, pts).hex() == u
    assert len(set(tuple(c["inv_length"][0]) for c in GOLDEN["scaffolds"])) > 1


# ---- a seeded synthetic case ------------------------------------------------------------------------------------------------------------------
def synthetic_case(seed, nmarkers=90, nsets=5, ndraws=12, span=60000):
    """(marker sets, positions, start lists, contig lengths): copies from none to five, a tenth of the markers without a key, markers in
    two co-located sets of a marker set, draws that are no multiples of their contig length, with repeated starts and an empty draw."""
    rng = random.Random(seed)
    names = ["m%03d" % k for k in range(nmarkers)]
    positions = {m: [[p, p + 300] for p in (rng.randrange(0, span) for _ in range(rng.choice([0, 1, 1, 1, 2, 3, 5])))] for m in names if rng.random() > 0.1}
    sets = []
    for s in range(nsets):
        mine = rng.sample(names, rng.randrange(1, nmarkers))
        cs, at = [], 0
        while at < len(mine):
            n = rng.choice([1, 1, 2, 3, 7])
            cs.append(set(mine[at:at + n]) | (set(rng.sample(mine, 1)) if rng.random() < 0.2 else set()))
            at += n
        sets.append(MarkerSet("UID%d" % s, "lineage%d" % (s % 3), 10 + s, cs))
    lens = [rng.choice([1, 700, 1000, 5000, 2**31 - 1]) for _ in range(ndraws)]
    starts = [sorted(rng.choice([rng.randrange(0, span), rng.randrange(0, span // 1000) * 1000]) for _ in range(rng.choice([0, 1, 5, 40, 200]))) for _ in range(ndraws)]
    starts[3] = []
    starts[4] = starts[4] + starts[4]
    return sets, positions, starts, lens


def test_host_executor_against_the_plain_loop(monkeypatch):
    use_host_executor(monkeypatch)
    b = MarkerSetBuilder(None)
    sets, positions, starts, lens = synthetic_case(3)
    want = b._genome_checks_host(sets, positions, starts, lens)
    got = b.genomeChecks(sets, positions, starts, lens)
    assert b.last_sim_timing["device"] and b.last_sim_timing["rounds"] == 1 and np.array_equal(got, want)
    assert len(set(want[:, :, 1].reshape(-1).tolist())) > 10 and want[3].tolist() == [[0.0] * 4] * len(sets) and want[:, :, 1].max() > 0
    tables = b._sim_tables(sets, positions, starts, lens)
    for budget, rounds in ((1, len(starts)), (4000, None), (1 << 30, 1)):
        r = emu.sim_run(None, tables, budget_bytes=budget)
        assert np.array_equal(r["out"], want) and (rounds is None or r["nrounds"] == rounds) and r["nrounds"] >= 1, budget
    assert 1 < emu.sim_run(None, tables, budget_bytes=4000)["nrounds"] < len(starts)
    empty = b.genomeChecks(sets, positions, [], [])
    assert empty.shape == (0, len(sets), 4)
    assert b.genomeChecks([], positions, starts, lens).shape == (len(starts), 0, 4)


def small_tables(**changes):
    t = dict(key_off=[0, 1, 3, 3], key=[10, 2500, 700], ms_off=[0, 2, 3], cs_off=[0, 2, 3, 5], cs_marker=[0, 1, 2, 1, 0], rs_off=[0, 2, 2, 5], starts=[0, 1000, 5, 5, 2000],
             contig_len=[1000, 1, 2**31 - 1])
    t.update(changes)
    return _lib.SimTables(**t)


def test_refusals():
    _lib.sim_check(small_tables())
    emu.sim_check(small_tables())
    assert emu.sim_run(None, small_tables())["out"].shape == (3, 2, 4)

    def refused(code, **changes):
        for check in (_lib.sim_check, emu.sim_check):
            with pytest.raises(_lib.CkmError) as e:
                check(small_tables(**changes))
            assert e.value.code == code, (check, changes)
    refused(-7, key=[10, 2**31, 700])
    refused(-7, key=[10, -1, 700])
    refused(-7, starts=[0, 1000, 5, 5, 2**31])
    refused(-7, starts=[-1, 1000, 5, 5, 2000])
    refused(-7, contig_len=[1000, 0, 5])
    refused(-7, contig_len=[1000, 1, 2**31])
    refused(-1, starts=[1000, 0, 5, 5, 2000])                      # not ascending within a replicate
    _lib.sim_check(small_tables(starts=[0, 1000, 5000, 5000, 6000]))                  # ascending within each replicate is enough
    _lib.sim_check(small_tables(starts=[0, 1000, 6000, 6000, 6000], rs_off=[0, 3, 3, 5]))
    refused(-1, key_off=[1, 1, 3, 3])
    refused(-1, key_off=[0, 2, 1, 3])
    refused(-1, key_off=[0, 1, 3, 4])                              # beyond the keys
    refused(-1, ms_off=[0, 2, 4])                                  # beyond the co-located sets
    refused(-1, rs_off=[0, 2, 2, 6])                               # beyond the starts
    refused(-1, rs_off=[0, 3, 2, 5])
    refused(-1, cs_off=[0, 2, 3, 6])                               # beyond the members
    refused(-1, cs_marker=[0, 1, 3, 1, 0])                         # a marker beyond the keys
    refused(-1, cs_off=[0, 2, 2, 5])                               # a co-located set of size 0
    refused(-1, ms_off=[0, 3, 3])                                  # a marker set with no sets
    with pytest.raises(_lib.CkmError):
        emu.sim_run(None, small_tables(ms_off=[0, 3, 3]))
    with pytest.raises(ValueError):
        small_tables(contig_len=[1000, 1])


def test_refused_calls_take_the_plain_loop(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(_lib, "sim_run", never)
    monkeypatch.setattr(runtime, "get_ctx", never)
    b = MarkerSetBuilder(None)
    ms = MarkerSet("U", "L", 3, [{"A", "B"}, {"C"}])
    far = {"A": [[2**31 + 10, 2**31 + 90]], "B": [[5, 9]], "C": [[2**40, 2**40 + 1], [2**40 + 1, 2**40 + 2]]}
    got = b.genomeChecks([ms], far, [[2**31, 2**40, 0]], [100])
    assert not b.last_sim_timing["device"] and got.tolist() == [[[100.0, 100 * 1.0 / 3, 100.0, 50.0]]]
    assert b.genomeChecks([ms], {"A": [[1.5, 2]]}, [[0]], [10]).tolist() == [[[100 * 1.0 / 3, 0.0, 25.0, 0.0]]]      # a position that is no integer
    assert b.genomeChecks([ms], {"A": [[5, 6]]}, [[0]], [5.5]).tolist() == [[[100 * 1.0 / 3, 0.0, 25.0, 0.0]]]        # a contig length that is no integer
    for broken in (MarkerSet("U", "L", 3, []), MarkerSet("U", "L", 3, [{"A"}, set()])):
        with pytest.raises(ZeroDivisionError):                     # the reference's own failure, before any launch
            b.genomeChecks([ms, broken], {"A": [[5, 6]]}, [[0]], [10])
    with pytest.raises(ValueError):
        b.genomeChecks([ms], far, [[0]], [10, 20])


def test_without_a_device_the_device_method_raises():
    b, call = MarkerSetBuilder(None), ([MarkerSet("U", "L", 3, [{"A"}])], {"A": [[5, 6]]}, [[0]], [10])
    if _lib.device_count() > 0:
        assert b.genomeChecks(*call).tolist() == [[[100.0, 0.0, 100.0, 0.0]]] and b.last_sim_timing["device"]
        return
    with pytest.raises(_lib.CkmError) as e:
        b.genomeChecks(*call)
    assert e.value.code == _lib.ENODEV


def test_header_and_exports_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    for n in ("ckm_sim_check", "ckm_sim_run"):
        assert n + "(" in header and n in _lib.EXPORTS and hasattr(_lib.load(), n)
    assert "#define CKM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.load().ckm_abi_version() == 12
    for line in ("scripts/simulation.py", ":353-369", ":206-238", "CKM_SIM_BATCH_MB", "ckm_sim_args;", "ckm_sim_info;"):
        assert line in header
    makefile = open(os.path.join(ROOT, "checkm_amd", "csrc", "Makefile")).read()
    for n in ("sim_host.o", "kernels_sim.o", "ckm_sim.o", "sim_dev.h"):
        assert n in makefile
