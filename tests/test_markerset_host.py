"""MarkerSetBuilder without a device: every golden case (tests/golden/markerset_cases.json, made by tools/gen_markerset_golden.py from the
reference's own IMG and markerSetBuilder.py) through checkm_amd.img.IMG, the host executor of the kernels' arithmetic (tests/emu/markerset)
and the host parts of checkm_amd.markerSetBuilder.MarkerSetBuilder, at ==; the host executor against a plain restatement of the pair test
on a seeded synthetic table; what the library refuses; the header and the export list."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd.img import IMG
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from tests.emu import markerset as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "markerset_cases.json")))["cases"]}


def all_files(c):
    """relative path -> text of every genome of a case: the files the golden holds, and the genomes that repeat another's under their own id"""
    out = dict(c["files"])
    for g, src in c["same_as"].items():
        out.update(("%s/%s%s" % (g, g, rel[len(src) * 2 + 1:]), text) for rel, text in c["files"].items() if rel.startswith(src + "/"))
    return out


def write_tree(d, c):
    for rel, text in all_files(c).items():
        p = os.path.join(d, *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    open(os.path.join(d, "tigrfam2pfam.tsv"), "w").write(c["redundant"])
    return d


def use_host_executor(monkeypatch):
    """The device entries of checkm_amd._lib replaced by the host executor; ckm_mset_check stays the library's (it needs no device)."""
    monkeypatch.setattr(_lib, "MsetTable", emu.MsetTable)
    monkeypatch.setattr(_lib, "mset_markers", emu.mset_markers)
    monkeypatch.setattr(_lib, "mset_colocated", emu.mset_colocated)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)


def run_case(c, d, batch=False):
    """The steps of tools/gen_markerset_golden.py: run_case with this package's classes: (out, printed, error) as the golden holds them.
    batch: buildMarkerSets over the case's list three times (with another list between) instead of buildMarkerSet."""
    img = IMG(os.path.join(d, "img_metadata.tsv"), os.path.join(d, "tigrfam2pfam.tsv"), genomeDir=write_tree(d, c))
    b = MarkerSetBuilder(img)
    ids, out, printed = c["genomeIds"], {}, io.StringIO()
    allIds = sorted(set(rel.split("/")[0] for rel in all_files(c)))
    try:
        with contextlib.redirect_stdout(printed):
            table = img.geneCountTable(allIds if c["cache"] else ids)
            out["count_table"] = table
            if c["cache"]:
                b.cachedGeneCountTable = table
            if "precompute_spacing" in c:
                img.precomputeGenomeSeqLens(ids)
                img.precomputeGenomeFamilyPositions(ids, c["precompute_spacing"])
                out["seq_lens"] = img.cachedGenomeSeqLens
            raw = b.markerGenes(ids, table, c["ubiquity"] * len(ids), c["single"] * len(ids))
            out["markers_raw"] = sorted(raw)
            out["tigr_removed"] = sorted(img.identifyRedundantTIGRFAMs(raw))
            out["pfam_redundant"] = sorted(img.identifyRedundantPFAMs(raw))
            markers = b.buildMarkerGenes(ids, c["ubiquity"], c["single"])
            out["markers"] = sorted(markers)
            dist = img.geneDistTable(ids, markers, c["spacing"])
            out["gene_dist_table"] = {g: {f: sorted(list(p) for p in copies) for f, copies in fams.items()} for g, fams in dist.items()}
            pairs = b.colocatedGenes(dist, c["dist_threshold"], c["genome_threshold"])
            assert pairs == sorted(pairs)
            out["pairs"] = pairs
            sets = b.colocatedSets(pairs, markers)
            assert sets == sorted(sets, key=min)
            out["sets"] = sorted(sorted(s) for s in sets)
            out["genome_check"] = {}
            for g in allIds:
                comp, cont, missing, dup = b.genomeCheck(sets, g, table)
                out["genome_check"][g] = [comp.hex(), cont.hex(), sorted(missing), sorted(dup)]
            b.cachedGeneCountTable = table
            out["missing"] = sorted(b.missingGenes(ids, markers, c["missing_threshold"]))
            out["duplicate"] = sorted(b.duplicateGenes(ids, markers, c["missing_threshold"]))
            if not c["cache"]:
                b.cachedGeneCountTable = None
            if batch:
                other = allIds[:1]
                got = b.buildMarkerSets([ids, other, ids, ids], c["ubiquity"], c["single"], c["spacing"])
                assert len(got) == 4 and got[1].numGenomes == len(other) and repr(got[0]) == repr(got[2]) == repr(got[3])
                ms = got[0]
            else:
                ms = b.buildMarkerSet(ids, c["ubiquity"], c["single"], c["spacing"])
            out["marker_set"] = dict(UID=ms.UID, lineageStr=ms.lineageStr, numGenomes=ms.numGenomes, sets=sorted(sorted(s) for s in ms.markerSet))
        error = None
    except (Exception, SystemExit) as e:
        error = dict(type=type(e).__name__, args=[repr(a) for a in e.args])
    return out, printed.getvalue(), error


def check_case(c, d, batch=False):
    out, printed, error = run_case(c, d, batch)
    assert error == c["error"], (c["name"], error)
    assert sorted(out) == sorted(c["out"]), c["name"]
    for k in sorted(out):
        assert out[k] == c["out"][k], (c["name"], k)
    if not batch:
        assert printed == c["printed"], c["name"]


# ---- a seeded synthetic table and the pair test restated plainly --------------------------------------------------------------------------
def synthetic_table(seed, G, C, span=20000):
    """count classes [G, C], pos_off, pos: about a fifth of the cells empty, copies up to 5, positions in [0, span) so that pairs within
    5000 are common, a few positions at the ends of the int32 range."""
    rng = np.random.default_rng(seed)
    ncopy = rng.choice([0, 1, 1, 1, 1, 1, 2, 3, 5], size=(G, C))
    cls = np.minimum(rng.choice([0, 1, 1, 1, 2, 5], size=(G, C)), 2).astype(np.uint8)
    pos_off = np.zeros(G * C + 1, dtype=np.uint64)
    np.cumsum(ncopy.reshape(-1), out=pos_off[1:])
    pos = rng.integers(0, span, size=int(pos_off[-1]), dtype=np.int64)
    if pos.size > 4:
        pos[:2] = (0, 2**31 - 1)
        pos[-2:] = (2**31 - 1, 2**31 - 4000)
    return cls, pos_off, pos


def plain_markers(cls, glist, tU, tS):
    out = []
    for f in range(cls.shape[1]):
        col = [int(cls[g, f]) for g in glist]
        u, s, d = sum(c > 0 for c in col), sum(c == 1 for c in col), sum(c > 1 for c in col)
        out.append((1 if u >= tU and s >= tS else 0) | (2 if len(glist) - u >= tU else 0) | (4 if d >= tU else 0))
    return out


def plain_colocated(cls, pos_off, pos, glist, mlist, D, thr):
    """(i, j, count) of the reported pairs of one query, i < j positions in mlist, ascending."""
    C, off, p = cls.shape[1], pos_off.tolist(), pos.tolist()
    copies = [[p[off[g * C + f]:off[g * C + f + 1]] for f in mlist] for g in glist]
    out = []
    for a in range(len(mlist)):
        for b in range(a + 1, len(mlist)):
            count = sum(1 for row in copies if any(abs(x - y) < D for x in row[a] for y in row[b]))
            if glist and float(count) / len(glist) > thr:
                out.append((a, b, count))
    return out


def triples(r, q):
    lo, hi = int(r["pair_off"][q]), int(r["pair_off"][q + 1])
    return list(zip(r["i"][lo:hi].tolist(), r["j"][lo:hi].tolist(), r["count"][lo:hi].tolist()))


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(name, tmp_path, monkeypatch):
    use_host_executor(monkeypatch)
    check_case(CASES[name], str(tmp_path))


@pytest.mark.parametrize("name", ["copies", "redundant_tigrfam", "empty_genome_list", "nineteen_of_twenty"])
def test_golden_case_as_a_batch(name, tmp_path, monkeypatch):
    use_host_executor(monkeypatch)
    check_case(CASES[name], str(tmp_path), batch=True)


def test_goldens_cover_what_they_must():
    c = CASES
    counts = set(v for fam in c["copies"]["out"]["count_table"].values() for v in fam.values())
    assert {1, 2, 5} <= counts and "pfam00007" not in str(c["copies"]["out"]["gene_dist_table"]) and "pfam00007" in c["copies"]["out"]["markers"]
    assert "\t0\n" in c["copies"]["files"]["G1/G1.gff"]                                   # the line of eight fields
    assert "pfam00001-pfam00002" in c["copies"]["out"]["pairs"] and "pfam00005-pfam00006" in c["copies"]["out"]["pairs"]
    assert len(c["contigs_spacing_0"]["out"]["pairs"]) == 3 and c["contigs_spacing_5000"]["out"]["pairs"] == ["pfam00011-pfam00012"]
    assert c["distance_edges"]["out"]["pairs"] == ["pfam00020-pfam00021", "pfam00021-pfam00022"]
    assert c["nineteen_of_twenty"]["out"]["pairs"] == ["pfam00030-pfam00031"] and c["ninetysix_of_hundred"]["out"]["pairs"] == ["pfam00040-pfam00041"]
    assert c["empty_genome_in_denominator"]["out"]["marker_set"]["sets"] == [["pfam00030"], ["pfam00031"], ["pfam00032"]]
    assert c["redundant_tigrfam"]["out"]["tigr_removed"] == ["TIGR00050"] and "TIGR00051" in c["redundant_tigrfam"]["out"]["markers"]
    assert c["empty_genome_list"]["printed"].count("degenerate") == 3 and len(c["empty_genome_list"]["out"]["markers"]) == 6
    assert c["contig_without_sequence"]["error"]["type"] == "KeyError"


def test_duplicate_genome_ids_take_the_plain_loop(tmp_path, monkeypatch):
    """A genome listed twice: ubiquity can exceed len(genomeCounts), the one place where the reference's early `continue` decides."""
    def never(*a, **k):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(_lib, "MsetTable", never)
    b = MarkerSetBuilder(None)
    table = {"pfamA": {"g1": 1}, "pfamB": {"g1": 1, "g2": 1, "g3": 2}}
    assert b.markerGenes(["g1", "g1", "g1"], table, 3, 3) == {"pfamB"}                   # pfamA: ubiquity 3, but len(genomeCounts) = 1 < 3
    assert b.markerGenes(["g1", "g1", "g2"], table, 3, 3) == {"pfamB"}
    b.cachedGeneCountTable = table
    assert b.duplicateGenes(["g3", "g3"], {"pfamA", "pfamB"}, 1.0) == {"pfamB"} and b.missingGenes(["g2", "g2"], {"pfamA"}, 0.5) == {"pfamA"}


def test_host_executor_against_the_plain_restatement():
    cls, pos_off, pos = synthetic_table(5, 70, 40)
    table = emu.MsetTable(None, cls, pos_off, pos)
    rng = np.random.default_rng(6)
    glists = [list(range(70)), [], [3], rng.permutation(70)[:33].tolist(), [69, 0]]
    mlists = [list(range(40)), [1, 2, 3], rng.permutation(40)[:17].tolist(), rng.permutation(40).tolist(), [5]]
    tU, tS = [0.5 * len(g) for g in glists], [0.3 * len(g) for g in glists]
    m = emu.mset_markers(None, table, glists, tU, tS, want_counts=True)
    for q, g in enumerate(glists):
        assert m["flag"][q].tolist() == plain_markers(cls, g, tU[q], tS[q])
        assert m["counts"][q, :, 0].tolist() == [sum(int(cls[x, f]) > 0 for x in g) for f in range(40)]
    want = [plain_colocated(cls, pos_off, pos, g, ml, 5000, 0.5) for g, ml in zip(glists, mlists)]
    assert sum(len(w) for w in want) > 50 and not want[1] and not want[4]
    one = emu.mset_colocated(None, table, glists, mlists, 5000, 0.5)
    assert [triples(one, q) for q in range(5)] == want and one["nbatches"] == 1 and one["nrounds"] == 1
    assert one["tests"] == sum(len(g) * len(ml) * (len(ml) - 1) // 2 for g, ml in zip(glists, mlists))
    for budget in (1, 100, 5000):
        cut = emu.mset_colocated(None, table, glists, mlists, 5000, 0.5, budget_bytes=budget)
        assert (cut["nbatches"] >= 3 or budget == 5000) and all(np.array_equal(cut[k], one[k]) for k in ("pair_off", "i", "j", "count")), budget
    assert emu.mset_colocated(None, table, glists, mlists, 5000, 0.5, budget_bytes=1)["nrounds"] == 3            # the queries with a pair to test
    # the threshold is strict, and 0 and 2^31 - 1 are thresholds like any other
    assert emu.mset_colocated(None, table, glists[:1], mlists[:1], 0, -1.0)["npairs"] == 40 * 39 // 2
    assert triples(emu.mset_colocated(None, table, glists[:1], mlists[:1], 0, 0.0), 0) == []
    far = emu.mset_colocated(None, table, glists[:1], mlists[:1], 2**31 - 1, 0.0)
    assert triples(far, 0) == plain_colocated(cls, pos_off, pos, glists[0], mlists[0], 2**31 - 1, 0.0)


def test_refusals():
    cls, pos_off, pos = synthetic_table(7, 4, 5)
    _lib.mset_check(cls, pos_off, pos, [[0, 1], []], [[0, 4], [2]], 5000)
    _lib.mset_check(cls, pos_off, pos, dist_threshold=5000.0)

    def refused(code, *a, **k):
        for check in (_lib.mset_check, emu.mset_check):
            with pytest.raises(_lib.CkmError) as e:
                check(*a, **k)
            assert e.value.code == code, (check, a)
    big = pos.copy(); big[3] = 2**31
    refused(-7, cls, pos_off, big)
    neg = pos.copy(); neg[3] = -1
    refused(-7, cls, pos_off, neg)
    refused(-1, cls, pos_off, pos, dist_threshold=4999.5)
    refused(-1, cls, pos_off, pos, dist_threshold=float("nan"))
    refused(-7, cls, pos_off, pos, dist_threshold=2.0**31)
    refused(-7, cls, pos_off, pos, dist_threshold=-1)
    shifted = pos_off.copy(); shifted[0] = 1
    refused(-1, cls, shifted, pos)
    falls = pos_off.copy(); falls[3] = falls[-1] + 5
    refused(-1, cls, falls, pos)
    three = cls.copy(); three[1, 1] = 3
    refused(-1, three, pos_off, pos)
    refused(-1, cls, pos_off, pos, [[0, 4]], None)                       # a genome beyond the table
    refused(-1, cls, pos_off, pos, [[0]], [[5]])                         # a family beyond the table
    with pytest.raises(_lib.CkmError):
        emu.MsetTable(None, cls, pos_off, big)


def test_refused_tables_and_thresholds_take_the_plain_loop(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the device was asked")
    monkeypatch.setattr(_lib, "MsetTable", never)
    b = MarkerSetBuilder(None)
    dist = {"g1": {"A": [[2**31, 2**31 + 900]], "B": [[2**31 + 4999, 2**31 + 5900]], "C": [[10, 20]]},
            "g2": {"A": [[100, 1000]], "B": [[5100, 6000]], "C": [[5099, 6000]]}}
    assert b.colocatedGenes(dist) == [] and b.colocatedGenes(dist, genomeThreshold=0.4) == ["A-B", "A-C", "B-C"]
    small = {"g1": {"A": [[100, 1000]], "B": [[5100, 6000]], "C": [[5099, 6000]]}}
    assert b.colocatedGenes(small, distThreshold=4999.5) == ["A-C", "B-C"] and b.colocatedGenes(small, distThreshold=5000.5) == ["A-B", "A-C", "B-C"]
    assert b.colocatedGenes({}) == [] and b.colocatedGenes({"g1": {"A": [[1, 2]]}}) == []


def test_colocated_genes_on_the_host_executor(monkeypatch):
    use_host_executor(monkeypatch)
    b = MarkerSetBuilder(None)
    small = {"g1": {"A": [[100, 1000]], "B": [[5100, 6000]], "C": [[5099, 6000], [90000, 90010]]}, "g2": {"C": [[5, 6]]}}
    assert b.colocatedGenes(small, genomeThreshold=0.4) == ["A-C", "B-C"] and b.colocatedGenes(small, 5001.0, 0.4) == ["A-B", "A-C", "B-C"]
    assert b.colocatedGenes(small) == []
    sets = b.colocatedSets(["B-C", "A-C", "X-Y"], {"A", "B", "C", "D", "X"})
    assert sets == [{"A", "B", "C"}, {"D"}, {"X", "Y"}]
    with pytest.raises(ValueError):
        b.colocatedSets(["A-B-C"], set())


def test_header_and_exports_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    names = ["ckm_mset_check", "ckm_mset_table_create", "ckm_mset_table_free", "ckm_mset_markers", "ckm_mset_colocated", "ckm_mset_columns_get", "ckm_mset_result_free"]
    for n in names:
        assert n + "(" in header and n in _lib.EXPORTS
    assert "#define CKM_ABI_VERSION 12" in header and "CKM_ABI_VERSION stays 12" in header and _lib.ABI_VERSION == 12
    assert _lib.load().ckm_abi_version() == 12
    for line in ("markerSetBuilder.py", ":131-157", ":159-192", ":486-510", ":512-536"):
        assert line in header
