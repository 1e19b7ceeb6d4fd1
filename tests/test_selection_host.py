"""The marker-set selection without a device: the generator's known answers; the host executor of the kernel's arithmetic
(tests/emu/selection) against the plain-Python draws of MarkerSetBuilder.sampledGenomeChecks at == on float64 bits; the exact properties
of every draw read from the returned multiplicities; the bridge from the multiplicities to the existing plain loop (_genome_checks_host);
the uniformity of both kinds of draw; every golden case (tests/golden/selection_cases.json, made by tools/gen_selection_golden.py from the
reference's own scripts) through MarkerSetSelection with draws='host', the two files byte for byte; what the library refuses; the header
and the export list."""
import json
import math
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib, runtime, selectDraws
from checkm_amd.img import IMG
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from checkm_amd.markerSetSelection import MarkerSetSelection
from checkm_amd.markerSets import BinMarkerSets, MarkerSet, MarkerSetParser
from checkm_amd.treeParser import read_newick
from tests.emu import markerset as mset_emu
from tests.emu import selection as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "selection_cases.json")))
EINVAL, ERANGE = -1, -7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(x, y):
    """Two results of select_run equal to the bit: truth, out and every multiplicity row."""
    return (np.array_equal(bits(x["truth"]), bits(y["truth"])) and np.array_equal(bits(x["out"]), bits(y["out"])) and not np.isnan(x["out"]).any()
            and not np.isnan(x["truth"]).any() and len(x["rows"]) == len(y["rows"]) and all(np.array_equal(a, b) for a, b in zip(x["rows"], y["rows"])))


def use_host_executor(monkeypatch):
    """The device entry of checkm_amd._lib replaced by the host executor; ckm_select_check stays the library's (it needs no device)."""
    monkeypatch.setattr(_lib, "select_run", emu.select_run)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)


def make_tables(genome_len, keys, sets, R, contig_len=1000, comp=(0.5, 1.0), cont=(0.0, 0.2), seed=1):
    """keys[g][m]: the positions of marker m in genome g; sets: marker sets as lists of co-located sets as lists of marker indices."""
    U = len(keys[0]) if keys else 0
    off = lambda lens: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)]) if len(lens) else np.zeros(1, dtype=np.uint64)
    cells = [c for g in keys for c in g]
    cs = [c for ms in sets for c in ms]
    return _lib.SelectTables(genome_len, U, off([len(c) for c in cells]), [p for c in cells for p in c], off([len(ms) for ms in sets]), off([len(c) for c in cs]),
                             [m for c in cs for m in c], R, contig_len, comp, cont, seed)


def random_sets(rng, U, S, max_sets=9, max_members=5):
    """S marker sets over U markers; a marker may sit in two co-located sets of one marker set."""
    return [[[int(m) for m in rng.randint(0, U, size=rng.randint(1, max_members + 1))] for _ in range(rng.randint(1, max_sets + 1))] for _ in range(S)]


def random_keys(rng, genome_len, U, contig_len, copies=(0, 1, 1, 1, 2, 5)):
    """Copies anywhere in the genome, in its partial tail and beyond its end."""
    return [[[int(rng.randint(0, n + 3 * contig_len)) for _ in range(rng.choice(copies))] for _ in range(U)] for n in genome_len]


def synthetic_tables(seed, genome_len=(20500, 64000, 1999, 257123), U=70, S=6, R=5, contig_len=1000, **kw):
    rng = np.random.RandomState(seed)
    return make_tables(list(genome_len), random_keys(rng, genome_len, U, contig_len), random_sets(rng, U, S), R, contig_len, seed=seed, **kw)


def builder_case(seed, sizes=(20500, 64000, 1999), nmarkers=40, nsets=4, contigLen=1000):
    """(marker sets, gene positions per genome, genome sizes) as sampledGenomeChecks takes them."""
    rng = np.random.RandomState(seed)
    markers = ["pfam%05d" % k for k in range(nmarkers)]
    sets = [MarkerSet(s, "UID%d | x" % s, 10, [set(markers[m] for m in c) for c in ms]) for s, ms in enumerate(random_sets(rng, nmarkers, nsets))]
    positions = [{m: [[p, p + 300] for p in c] for m, c in zip(markers, g) if c} for g in random_keys(rng, sizes, nmarkers, contigLen)]
    return sets, positions, list(sizes)


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % w for w in emu.philox(counter, key)) == want
    assert " ".join("%08x" % int(w[0]) for w in selectDraws.philox4x32(counter, key)) == want


def test_unit_is_in_the_half_open_interval():
    assert emu.unit(0, 0) == 0.0 and emu.unit(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 < 1.0
    rng = random.Random(3)
    for _ in range(2000):
        a, b = rng.getrandbits(32), rng.getrandbits(32)
        u = emu.unit(a, b)
        assert 0.0 <= u < 1.0 and u == selectDraws.unit(a, b) == ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0


def test_the_words_of_a_draw_depend_on_its_counter_alone():
    w = selectDraws.words(77, selectDraws.STREAM_COMP, 3, 9, 10)
    assert [int(x) for x in w[4:8]] == emu.philox((1, 9, 3, 1), (77, 0))
    assert [int(x) for x in selectDraws.words((5 << 32) | 77, selectDraws.STREAM_CONT, 3, 9, 3)] == emu.philox((0, 9, 3, 2), (77, 5))[:3]


# ---- the executor against the plain-Python path ---------------------------------------------------------------------------------------------------
def test_host_executor_against_the_plain_python_draws(monkeypatch):
    use_host_executor(monkeypatch)
    b = MarkerSetBuilder(None)
    sets, positions, sizes = builder_case(11)
    for comp, cont, seed in (((0.5, 1.0), (0.0, 0.2), 0), ((0.0, 1.0), (0.0, 3.0), (1 << 63) + 12345), ((1.0, 1.0), (0.0, 0.0), 7)):
        true, out, mults = b.sampledGenomeChecks(sets, positions, sizes, 6, 1000, comp, cont, seed, withDraws=True)
        assert b.last_select_timing["device"] and b.last_select_timing["rounds"] == 1
        want = b._sampled_checks_host(sets, positions, sizes, 6, 1000, comp, cont, seed)
        assert np.array_equal(bits(true), bits(want[0])) and np.array_equal(bits(out), bits(want[1])) and true.shape == (3, 6, 2) and out.shape == (3, 6, len(sets), 4)
        assert all(np.array_equal(a, w) and a.dtype == np.uint16 for a, w in zip(mults, want[2])) and [m.shape for m in mults] == [(6, 20), (6, 64), (6, 1)]
        assert (out[:, :, :, 0] > 0).any()
        assert [x.shape for x in b.sampledGenomeChecks(sets, positions, sizes, 6, 1000, comp, cont, seed)] == [(3, 6, 2), (3, 6, len(sets), 4)]


def test_every_draw_has_the_stated_counts():
    t = synthetic_tables(5, R=40, comp=(0.0, 1.0), cont=(0.0, 2.0))
    r = emu.select_run(None, t, with_rows=True)
    for g, (n, rows) in enumerate(zip(t.genome_len.tolist(), r["rows"])):
        C = n // t.contig_len
        for rep in range(t.nreplicates):
            f = emu.philox((0, rep, g, 0), (t.seed & 0xffffffff, t.seed >> 32))
            testComp, testCont = t.comp_lo + (t.comp_hi - t.comp_lo) * emu.unit(f[0], f[1]), t.cont_lo + (t.cont_hi - t.cont_lo) * emu.unit(f[2], f[3])
            nComp, nCont = int(C * testComp + 0.5), int(C * testCont + 0.5)
            assert (nComp, nCont) == selectDraws.plan(t.seed, g, rep, n, t.contig_len, (t.comp_lo, t.comp_hi), (t.cont_lo, t.cont_hi))[:2]
            assert r["truth"][g, rep].tolist() == [float(nComp) * t.contig_len * 100 / n, float(nCont) * t.contig_len * 100 / n]
            assert int(rows[rep].sum()) == nComp + nCont
            # the completeness contigs: the nComp smallest (word, index) pairs, each once; what is left are the contamination draws
            w = selectDraws.words(t.seed, selectDraws.STREAM_COMP, g, rep, C)
            taken = sorted(range(C), key=lambda i: (int(w[i]), i))[:nComp]
            cont = rows[rep].astype(np.int64)
            assert (cont[taken] >= 1).all()
            cont[taken] -= 1
            landing = [(int(x) * C) >> 32 for x in selectDraws.words(t.seed, selectDraws.STREAM_CONT, g, rep, nCont)]
            assert cont.tolist() == np.bincount(np.asarray(landing, dtype=np.int64), minlength=C).tolist()


def test_equal_words_are_ranked_by_contig_index():
    """The threshold pair where words repeat: C = 1 and C = 2 cannot show it, so the rule is checked on the pair order itself."""
    w = np.array([5, 3, 5, 3, 9], dtype=np.uint64)
    pairs = (w << np.uint64(32)) | np.arange(5, dtype=np.uint64)
    assert np.argsort(pairs, kind="stable").tolist() == [1, 3, 0, 2, 4] == sorted(range(5), key=lambda i: (int(w[i]), i))


TIE_SEED, TIE_CONTIGS, TIE_RANK = 11, (5162, 11795), 10623


def tied_tables(ncomp):
    """Draw (genome 0, replicate 0) of seed 11 over 16384 contigs: contigs 5162 and 11795 get the same word, and 10623 words are smaller.
    With nComp = 10624 the threshold pair is the first of the two, and the contig index decides."""
    C = 16384
    return make_tables([C * 10], [[[51620, 117950, 7]]], [[[0]]], 1, 10, (ncomp / C, ncomp / C), (0.0, 0.0), TIE_SEED)


def test_a_threshold_word_that_two_contigs_share():
    w = selectDraws.words(TIE_SEED, selectDraws.STREAM_COMP, 0, 0, 16384)
    assert int(w[TIE_CONTIGS[0]]) == int(w[TIE_CONTIGS[1]]) and int((w < w[TIE_CONTIGS[0]]).sum()) == TIE_RANK and int((w == w[TIE_CONTIGS[0]]).sum()) == 2
    for ncomp, first, second in ((TIE_RANK + 1, 1, 0), (TIE_RANK + 2, 1, 1), (TIE_RANK, 0, 0)):
        row = emu.select_run(None, tied_tables(ncomp), with_rows=True)["rows"][0][0]
        assert (int(row[TIE_CONTIGS[0]]), int(row[TIE_CONTIGS[1]])) == (first, second) and int(row.sum()) == ncomp
        assert np.array_equal(row, np.minimum(selectDraws.draw(TIE_SEED, 0, 0, 163840, 10, (ncomp / 16384,) * 2, (0.0, 0.0))[2], 65535))


def test_bridge_from_the_multiplicities_to_the_plain_loop():
    """mult[p / contigLen] against containedMarkerGenes on the starts c * contigLen, copies in the partial tail and beyond the end included."""
    b = MarkerSetBuilder(None)
    sets, positions, sizes = builder_case(23, sizes=(20999, 5000, 64001))
    positions[0][sets[0].getMarkerGenes().pop()] = [[0, 10], [20000, 20100], [20998, 21100], [20999, 21100], [50000, 50100], [19999, 20100]]
    t = b._select_tables(sets, positions, sizes, 8, 1000, (0.3, 1.0), (0.0, 1.5), 99)
    r = emu.select_run(None, t, with_rows=True)
    for g in range(len(sizes)):
        for rep in range(8):
            starts = selectDraws.contig_starts(r["rows"][g][rep], 1000)
            assert starts == sorted(starts) and len(starts) == int(r["rows"][g][rep].sum())
            want = b._genome_checks_host(sets, positions[g], [starts], [1000])[0]
            assert np.array_equal(bits(r["out"][g, rep]), bits(want))
    assert (r["out"] > 0).any(axis=(0, 1, 2)).all()


@pytest.fixture(scope="module")
def uniform_draws():
    """20000 draws of 32 of 64 contigs, once without replacement (completeness alone) and once with (contamination alone)."""
    one = lambda comp, cont: emu.select_run(None, make_tables([64 * 10 + 3], [[[5]]], [[[0]]], 20000, 10, comp, cont, seed=2024), with_rows=True)["rows"][0]
    return one((0.5, 0.5), (0.0, 0.0)), one((0.0, 0.0), (0.5, 0.5))


def test_completeness_draws_are_uniform(uniform_draws):
    rows = uniform_draws[0]
    assert rows.shape == (20000, 64) and rows.max() == 1 and (rows.sum(axis=1) == 32).all()
    counts = rows.sum(axis=0, dtype=np.int64)
    sigma = math.sqrt(20000 * 0.25)
    assert abs(counts - 10000).max() <= 425 and 425 >= 6 * sigma > 424, counts


def test_contamination_draws_are_uniform(uniform_draws):
    rows = uniform_draws[1]
    assert (rows.sum(axis=1) == 32).all() and rows.max() > 1
    counts = rows.sum(axis=0, dtype=np.int64)
    sigma = math.sqrt(20000 * 32 * (1 / 64) * (63 / 64))
    assert abs(counts - 10000).max() <= 600 and 99 < sigma < 100 and 6 * sigma <= 600, counts


def test_rounds_never_change_a_result():
    t = synthetic_tables(8)
    one = emu.select_run(None, t, with_rows=True)
    assert one["nrounds"] == 1
    draws = t.ngenomes * t.nreplicates
    for budget, rounds in ((1, draws), (3000, None)):
        r = emu.select_run(None, t, budget_bytes=budget, with_rows=True)
        assert same(r, one) and (r["nrounds"] == rounds if rounds else 1 < r["nrounds"] < draws)
    assert same(dict(emu.select_run(None, t, budget_bytes=1), rows=[]), dict(one, rows=[]))
    other = emu.select_run(None, synthetic_tables(8, comp=(0.5, 1.0)), with_rows=True)
    assert same(other, one)
    t.seed += 1
    assert not all(np.array_equal(a, b) for a, b in zip(emu.select_run(None, t, with_rows=True)["rows"], one["rows"]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def small_tables(**changes):
    a = dict(genome_len=[10500, 3000], keys=[[[10, 700], [], [9000]], [[5], [2999, 3000], []]], sets=[[[0, 1], [2]], [[1, 1, 2]]], R=3, contig_len=1000, comp=(0.5, 1.0),
             cont=(0.0, 0.2), seed=4)
    a.update(changes)
    t = make_tables(a["genome_len"], a["keys"], a["sets"], a["R"], a["contig_len"], a["comp"], a["cont"], a["seed"])
    for name in ("key_off", "ms_off", "cs_off", "cs_marker"):
        if name in changes:
            dtype = np.uint32 if name == "cs_marker" else np.uint64
            setattr(t, name, np.ascontiguousarray(changes[name], dtype=dtype))
    return t


REFUSED = [(ERANGE, dict(genome_len=[16385 * 1000, 3000])), (ERANGE, dict(genome_len=[10500, 999])), (ERANGE, dict(genome_len=[10500, 0])), (ERANGE, dict(contig_len=0)),
           (ERANGE, dict(contig_len=1 << 31)), (ERANGE, dict(comp=(0.5, 1.0000001))), (ERANGE, dict(comp=(-0.1, 1.0))), (ERANGE, dict(comp=(0.9, 0.8))),
           (ERANGE, dict(comp=(0.5, float("nan")))), (ERANGE, dict(cont=(0.0, 8.5))), (ERANGE, dict(cont=(0.0, float("inf")))), (ERANGE, dict(cont=(0.3, 0.2))),
           (ERANGE, dict(genome_len=[16384 * 1000, 3000], cont=(0.0, 4.0))),                      # 65536 contamination draws
           (ERANGE, dict(genome_len=[16384 * 1000, 3000], cont=(0.0, 3.9), keys=[[[10] * 70000, [], []], [[5], [], []]])),      # 70000 copies x 63899 draws
           (ERANGE, dict(keys=[[[10, 1 << 31], [], [9000]], [[5], [2999], []]])), (ERANGE, dict(keys=[[[10, -1], [], [9000]], [[5], [2999], []]])),
           (EINVAL, dict(key_off=[0, 2, 1, 3, 4, 6, 6])), (EINVAL, dict(key_off=[0, 2, 2, 3, 4, 6, 7])), (EINVAL, dict(key_off=[1, 2, 2, 3, 4, 6, 6])),
           (EINVAL, dict(ms_off=[0, 2, 2])), (EINVAL, dict(cs_off=[0, 2, 2, 6])), (EINVAL, dict(cs_marker=[0, 1, 2, 1, 3, 2])), (EINVAL, dict(ms_off=[0, 2, 4]))]


@pytest.mark.parametrize("code,changes", REFUSED)
def test_refusals(code, changes):
    for check in (_lib.select_check, emu.select_check):
        with pytest.raises(_lib.CkmError) as e:
            check(small_tables(**changes))
        assert e.value.code == code
    with pytest.raises(_lib.CkmError):
        emu.select_run(None, small_tables(**changes))


def test_just_legal_calls_pass():
    _lib.select_check(small_tables())
    assert emu.select_run(None, small_tables())["out"].shape == (2, 3, 2, 4)
    for changes in (dict(genome_len=[16384 * 1000 + 999, 3000]), dict(genome_len=[16384 * 1000, 3000], cont=(0.0, 3.99993)), dict(comp=(0.0, 0.0), cont=(8.0, 8.0)),
                    dict(comp=(1.0, 1.0)), dict(keys=[[[0, (1 << 31) - 1], [], [9000]], [[5], [2999], []]]), dict(R=0)):
        _lib.select_check(small_tables(**changes))
        emu.select_check(small_tables(**changes))
    assert "16384" in _lib_error(dict(genome_len=[16385 * 1000, 3000])) and "65535" in _lib_error(dict(genome_len=[16384 * 1000, 3000], cont=(0.0, 4.0)))


def _lib_error(changes):
    with pytest.raises(_lib.CkmError) as e:
        _lib.select_check(small_tables(**changes))
    return str(e.value)


def test_refused_calls_take_the_plain_python_path(monkeypatch):
    """One contig more than a block keeps: the Python path answers, with the numbers the executor gives the just-legal neighbour where the
    two calls make the same draws (the second genome: same length, same counter, same key)."""
    def never(*a, **k):
        raise AssertionError("the device was asked")
    b = MarkerSetBuilder(None)
    sets, positions, _ = builder_case(31, sizes=(5000, 5000))
    monkeypatch.setattr(runtime, "get_ctx", never)
    monkeypatch.setattr(_lib, "select_run", never)
    refused = b.sampledGenomeChecks(sets, positions, [16385 * 10, 5000], 3, 10, (0.5, 1.0), (0.0, 0.2), 6, withDraws=True)
    assert not b.last_select_timing["device"] and refused[2][0].shape == (3, 16385)
    use_host_executor(monkeypatch)
    legal = b.sampledGenomeChecks(sets, positions, [16384 * 10, 5000], 3, 10, (0.5, 1.0), (0.0, 0.2), 6, withDraws=True)
    assert b.last_select_timing["device"] and legal[2][0].shape == (3, 16384)
    assert np.array_equal(bits(refused[0][1]), bits(legal[0][1])) and np.array_equal(bits(refused[1][1]), bits(legal[1][1])) and np.array_equal(refused[2][1], legal[2][1])
    assert int(refused[2][0].sum()) > 3 * 8000
    # a position beyond int32 is refused as well, and the Python path counts it like any other
    monkeypatch.setattr(_lib, "select_run", never)
    positions[1][sets[0].getMarkerGenes().pop()] = [[1 << 31, (1 << 31) + 10], [1200, 1300]]
    true, out = b.sampledGenomeChecks(sets, positions, [5000, 5000], 3, 10, (0.5, 1.0), (0.0, 0.2), 6)
    assert not b.last_select_timing["device"] and np.array_equal(bits(true[1]), bits(legal[0][1]))


def test_header_and_exports_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    assert "#define CKM_ABI_VERSION 12" in header
    for name in ("ckm_select_check", "ckm_select_run"):
        assert name in header and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    make = open(os.path.join(ROOT, "checkm_amd", "csrc", "Makefile")).read()
    assert "select_dev.h" in make and all("$(OBJDIR)/%s.o" % n in make for n in ("select_host", "kernels_select", "ckm_select"))


# ---- MarkerSetSelection against the reference's scripts -----------------------------------------------------------------------------------------------
def write_case(d, c):
    files = dict(c["files"])
    for g, src in c["same_as"].items():
        files.update(("%s/%s%s" % (g, g, rel[len(src) * 2 + 1:]), text) for rel, text in c["files"].items() if rel.startswith(src + "/"))
    for rel, text in files.items():
        p = os.path.join(str(d), *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    for name, key in (("tigrfam2pfam.tsv", "redundant"), ("metadata.tsv", "metadata"), ("derep.txt", "derep"), ("missing_duplicate.tsv", "missing_duplicate")):
        open(os.path.join(str(d), name), "w").write(c[key])


def selection_of(d, monkeypatch):
    """(MarkerSetSelection over the golden genome directory, its tree, the internal nodes with a parent in the script's order).  With
    monkeypatch the marker pass, the simulation pass and the selection pass run on their host executors."""
    write_case(d, GOLDEN)
    b = MarkerSetBuilder(IMG(None, os.path.join(str(d), "tigrfam2pfam.tsv"), str(d)))
    b.readNodeMetadata(os.path.join(str(d), "metadata.tsv"))
    b.readDuplicateSeqs(os.path.join(str(d), "derep.txt"))
    b.readLineageSpecificGenesToRemove(os.path.join(str(d), "missing_duplicate.tsv"))
    if monkeypatch is not None:
        from tests.emu import simulation as sim_emu
        for n in ("MsetTable", "mset_markers", "mset_colocated"):
            monkeypatch.setattr(_lib, n, getattr(mset_emu, n))
        monkeypatch.setattr(_lib, "sim_run", sim_emu.sim_run)
        use_host_executor(monkeypatch)
    tree = read_newick(GOLDEN["newick"])
    by_label = {}
    stack = [tree.root]
    while stack:
        n = stack.pop()
        by_label[n.label] = n
        stack.extend(n.children)
    return MarkerSetSelection(b, simContigLen=GOLDEN["simContigLen"]), tree, [by_label[n["label"]] for n in GOLDEN["nodes"]]


def as_golden(t):
    return tuple(x if isinstance(x, (str, int)) or x is None else float(x).hex() for x in t)


def wanted_tuples(sel, tree, nodes, draws):
    """selectMarkerSet per node, both generators seeded with the node's recorded seed as the golden tool seeded the script's."""
    out = []
    for node, g in zip(nodes, GOLDEN["nodes"]):
        random.seed(g["seed"])
        np.random.seed(g["seed"] & 0xffffffff)
        out.append(as_golden(sel.selectMarkerSet(tree, node, GOLDEN["ubiquity"], GOLDEN["single"], draws=draws, seed=g["seed"])))
    return out


def test_golden_holds_what_the_issue_asks():
    tuples = [n["tuple"] for n in GOLDEN["nodes"]]
    assert len(tuples) == 9 and sum(t[0] != "NA" for t in tuples) == 2 and ["NA", -1, -1, -1, -1, -1] in tuples
    assert all(t[1].endswith(" ") for t in tuples if t[0] != "NA")                       # the trailing blank of lineageStr.split('|')[0]
    assert GOLDEN["table"].count("\n") == 3 and GOLDEN["selected"].count("\n") == 10 and "test genomes sampled from the sorted child" in GOLDEN["substitutions"]["simInferBestMarkerSet"]
    assert "UID10\tUID2\n" in GOLDEN["selected"] and GOLDEN["selected"] != GOLDEN["edited_selected"]


def test_select_marker_set_with_host_draws_gives_the_reference_tuples(monkeypatch, tmp_path):
    sel, tree, nodes = selection_of(tmp_path, monkeypatch)
    assert wanted_tuples(sel, tree, nodes, "host") == [tuple(n["tuple"]) for n in GOLDEN["nodes"]]
    assert sel.markerSetBuilder.last_sim_timing["device"]                                    # scored by genomeChecks' device path (here: its executor)
    with pytest.raises(ValueError):
        sel.selectMarkerSet(tree, nodes[0], 0.8, 0.8, draws="numpy")


def test_run_writes_the_reference_table_and_the_mapping(monkeypatch, tmp_path):
    sel, tree, nodes = selection_of(tmp_path, monkeypatch)
    assert [MarkerSetSelection.node_seed(GOLDEN["seed"], n) for n in nodes] == [g["seed"] for g in GOLDEN["nodes"]]
    table, selected = str(tmp_path / "simInferBestMarkerSet.tsv"), str(tmp_path / "selected_marker_sets.tsv")
    chains = []
    whole = sel.markerSetBuilder._chains
    monkeypatch.setattr(sel.markerSetBuilder, "_chains", lambda *a, **k: chains.append(len(a[0])) or whole(*a, **k))
    results = sel.run(tree, GOLDEN["ubiquity"], GOLDEN["single"], table, draws="host", seed=GOLDEN["seed"])
    assert chains == [2]                                                                     # the chains of all eligible nodes from one call
    assert open(table).read() == GOLDEN["table"] and [as_golden(t) for t in results] == [tuple(n["tuple"]) for n in GOLDEN["nodes"]]
    assert sel.last_timing["nodes"] == 2 and sel.last_timing["draws_made"] == 2 * 5 * 100
    want = sel.selectedMarkerSetMap(tree, table, selected)
    assert open(selected).read() == GOLDEN["selected"]
    from checkm_amd.defaultValues import DefaultValues
    monkeypatch.setattr(DefaultValues, "SELECTED_MARKER_SETS", selected)
    assert MarkerSetParser().parseSelectedMarkerSetMap() == want and want["UID5"] == "UID3" and want["UID12"] == "UID2"
    # a table with an 'NA' set and a set given with its lineage string
    open(table, "w").write(GOLDEN["edited_table"])
    sel.selectedMarkerSetMap(tree, table, selected)
    assert open(selected).read() == GOLDEN["edited_selected"]


def test_device_draws_through_the_executor(monkeypatch, tmp_path):
    """draws='device' on the host executor: deterministic in the seed, no use of Python's generators for the draws, a set chosen."""
    sel, tree, nodes = selection_of(tmp_path, monkeypatch)
    first = wanted_tuples(sel, tree, nodes, "device")
    assert sel.markerSetBuilder.last_select_timing["device"] and first == wanted_tuples(sel, tree, nodes, "device")
    picked = [t for t in first if t[0] != "NA"]
    assert len(picked) == 2 and all(t[1] in ("UID2 ", "UID3 ", "UID7 ") and 0 < float.fromhex(t[2]) < 50 for t in picked)
    assert [t[0] for t in first] == [n["tuple"][0] for n in GOLDEN["nodes"]]
    table = str(tmp_path / "device.tsv")
    a = sel.run(tree, GOLDEN["ubiquity"], GOLDEN["single"], table, seed=1)
    b = sel.run(tree, GOLDEN["ubiquity"], GOLDEN["single"], table, seed=1)
    assert [as_golden(t) for t in a] == [as_golden(t) for t in b] != [as_golden(t) for t in sel.run(tree, GOLDEN["ubiquity"], GOLDEN["single"], table, seed=2)]
    assert open(table).read().startswith(MarkerSetSelection.HEADER) and open(table).read().count("\n") == 3


def test_a_child_of_four_genomes_gives_na_and_ties_keep_the_first_set(monkeypatch, tmp_path):
    sel, tree, nodes = selection_of(tmp_path, monkeypatch)
    uid10 = [n for n in nodes if n.label.startswith("UID10|")][0]
    assert len(sel._smallest_child(uid10)) == 4 and sel.selectMarkerSet(tree, uid10, 0.8, 0.8, draws="host") == ("NA", -1, -1, -1, -1, -1)
    uid7 = [n for n in nodes if n.label.startswith("UID7|")][0]
    assert len(sel._smallest_child(uid7)) == 5 and "C5" in sel._smallest_child(uid7)         # the dereplicated genome counts
    chain, _ = sel.markerSetBuilder.buildBinMarkerSet(tree, uid7, 0.8, 0.8, bMarkerSet=False, genomeIdsToRemove=sel._smallest_child(uid7))
    first = list(chain.markerSetIter())[0]
    for names in (("UID900 | twin", "UID901 | twin"), ("UID901 | twin", "UID900 | twin")):
        tied = BinMarkerSets(uid7.label, BinMarkerSets.TREE_MARKER_SET)
        for name in names:
            tied.addMarkerSet(MarkerSet(0, name, first.numGenomes, [set(cs) for cs in first.markerSet]))
        for draws in ("host", "device"):
            random.seed(5)
            np.random.seed(5)
            got = sel.selectMarkerSet(tree, uid7, 0.8, 0.8, draws=draws, seed=5, repsPerGenome=10, chain=tied)
            assert got[1] == names[0].split("|")[0] and got[2] > 0
