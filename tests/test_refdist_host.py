"""ReferenceDistributions without a device: the plain-Python restatement (tests/refdist_reference.py) against the goldens made from the
reference's own primitives (tests/golden/refdist_cases.json), and the host executor (tests/emu/refdist_emu.cpp: refdist_dev.h's
geometry, seqwin_dev.h's lane step, outlier_dev.h's distance) plus the library's real host code (reader, argument check, coding
lookups) against the restatement.  Everything is compared at ==, floats by float.hex()."""
import json
import logging
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib, common, runtime
from checkm_amd import referenceDistributions as rdm
from checkm_amd.defaultValues import DefaultValues
from tests import refdist_reference as ref
from tests.emu import refdist as emu
from tests.seqwin_reference import read_fasta, tetra_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "refdist_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
RUNS = [(c["name"], stat) for c in GOLD["cases"] for stat in c["stats"]]
BLOCKS = [16, 17, 64, 256]


def hexes(v):
    return [float(x).hex() for x in v]


def outcome(fn):
    """dict(error, head, dist) as the goldens hold them."""
    try:
        with np.errstate(invalid="ignore"):
            head, dist = fn()
    except (ValueError, ZeroDivisionError) as e:
        return dict(error=type(e).__name__, message=str(e))
    return dict(error=None, head=hexes(head) if np.ndim(head) else float(head).hex(), dist={str(w): hexes(v) for w, v in dist.items()})


def expect(case, stat):
    g = case["results"][stat]
    if g["error"]:
        out = dict(error=g["error"]["type"])
        if g["error"]["type"] == "ValueError":
            out["message"] = str(ref.no_window_error(case["name"], stat, int(g["error"]["args"][2]), case["numWindows"]))
        return out
    return dict(error=None, head=g["head"], dist=g["dist"])


def trim(o):
    if o["error"] == "ZeroDivisionError":
        o = dict(error=o["error"])
    return o


def write_case(d, case):
    path, gff = str(d / (case["name"] + ".fna")), str(d / (case["name"] + ".gff"))
    open(path, "w").write(case["fasta"])
    if case["gff"] is not None:
        open(gff, "w").write(case["gff"])
    return path, gff


def restated(case, stat):
    seqs = read_fasta(case["fasta"])
    n, sizes, seed, gid = case["numWindows"], case["sizes"], case["seed"], case["name"]
    if stat == "gc":
        return ref.delta_gc(seqs, gid, n, sizes, seed)
    if stat == "td":
        return ref.delta_td(seqs, gid, n, sizes, seed)
    return ref.delta_cd(seqs, case["gff"], gid, n, sizes, seed)


def through_class(R, case, stat, path, gff):
    n, sizes, seed = case["numWindows"], case["sizes"], case["seed"]
    if stat == "gc":
        return R.deltaGC(path, n, sizes, seed)
    if stat == "td":
        return R.deltaTD(path, n, sizes, seed)
    return R.deltaCD(path, gff, n, sizes, seed)


@pytest.fixture
def host_executor(monkeypatch):
    emu.build()
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    monkeypatch.setattr(_lib, "refdist", emu.refdist)


def test_window_sizes_are_the_scripts():
    sizes = ref.window_sizes()
    want = []
    for a in (np.arange(500, 1000, 100), np.arange(1000, 2000, 200), np.arange(2000, 5000, 500), np.arange(5000, 10000, 1000), np.arange(10000, 50000, 5000),
              np.arange(50000, 100000, 10000), np.arange(100000, 400000, 100000), np.arange(400000, 1000001, 200000)):
        want += a.tolist()
    assert sizes == want and len(sizes) == 41 and sizes == sorted(sizes) and rdm.ReferenceDistributions().windowSizes() == sizes


@pytest.mark.parametrize("name,stat", RUNS)
def test_restatement_reproduces_the_goldens(name, stat):
    case = CASES[name]
    assert trim(outcome(lambda: restated(case, stat))) == expect(case, stat)
    g = case["results"][stat]
    if not g["error"]:
        head, dist = restated(case, stat)
        assert ref.file_text(stat, head, dist) == g["file"]
    assert ref.scaffold_file(read_fasta(case["fasta"]), name) == case["scaffold_file"]


def test_goldens_hold_the_edge_cases():
    m = CASES["mixed"]
    L = len(ref.scaffold(read_fasta(m["fasta"]), "gc"))
    assert str(L - 1) in m["results"]["gc"]["dist"] and str(L) not in m["results"]["gc"]["dist"] and "500" not in m["results"]["gc"]["dist"]
    assert "nan" in m["results"]["td"]["dist"]["3"] and set(m["results"]["td"]["dist"]["1"]) == {"nan"}
    assert any("nan" in v for w, v in m["results"]["td"]["dist"].items() if int(w) >= 4)
    # GC acceptance exactly at the threshold: only the windows with 9 of 10 (450 of 500) bases are there
    t10 = read_fasta(CASES["t10"]["fasta"])["t"]
    assert sorted(set(ref.gc_at(t10[s:s + 10].upper())[0] + ref.gc_at(t10[s:s + 10].upper())[1] for s in range(3))) == [8, 9]
    assert len(CASES["t10"]["results"]["gc"]["dist"]["10"]) == CASES["t10"]["numWindows"]
    t500 = read_fasta(CASES["t500"]["fasta"])["t"]
    assert [sum(ref.gc_at(t500[s:s + 500])) for s in range(2)] == [449, 450] and len(set(CASES["t500"]["results"]["gc"]["dist"]["500"])) == 1
    assert CASES["gc_never"]["results"]["gc"]["error"]["args"][2] == "20" and CASES["cd_never"]["results"]["cd"]["error"]["args"][2] == "151"


@pytest.mark.parametrize("name,stat", RUNS)
def test_class_on_the_host_executor_reproduces_the_goldens(host_executor, tmp_path, name, stat):
    case = CASES[name]
    path, gff = write_case(tmp_path, case)
    for block in (0, 16, 17):
        R = rdm.ReferenceDistributions()
        R.block = block
        assert trim(outcome(lambda: through_class(R, case, stat, path, gff))) == expect(case, stat)
    R.writeScaffold(path, str(tmp_path / "scaffold.fna"))
    assert open(str(tmp_path / "scaffold.fna")).read() == case["scaffold_file"]


def random_genome(r, lens, dirty=True):
    seqs = []
    for n in lens:
        s = "".join(r.choice("ACGT") for _ in range(n))
        if dirty:
            s = list(s)
            for _ in range(n // 9):
                s[r.randrange(n)] = r.choice("acgtUuNnRY")
            if n > 60:
                a = r.randrange(n - 40)
                s[a:a + 23] = "N" * 23
            s = "".join(s)
        seqs.append(s)
    return seqs


def window_shapes(r, L, block):
    """(starts, sizes): every shape of a window against the blocks, and a few at random."""
    st, sz = [], []
    for w in (1, 3, 4, 5, block - 1, block, block + 1, 2 * block, 2 * block + 3, 3 * block + 2, L - 1, L):
        if w < 1 or w > L:
            continue
        for s in {0, L - w, block, 2 * block, block - 1, block + 1, 3 * block - w, 2 * block - w + 1, r.randint(0, L - w), r.randint(0, L - w)}:
            if 0 <= s <= L - w:
                st.append(s)
                sz.append(w)
    return st, sz


def restated_windows(scaf, stat, st, sz):
    if stat == "td":
        with np.errstate(invalid="ignore"):
            sig = ref.signature(scaf)
            return hexes(np.sum(np.abs(sig - ref.signature(scaf[s:s + w]))) for s, w in zip(st, sz))
    return [list(ref.gc_at(scaf[s:s + w])) for s, w in zip(st, sz)]


def run_windows(fn, ctx, tmp_path, seqs, stat, st, sz, tag="g", **kw):
    path = str(tmp_path / (tag + ".fna"))
    open(path, "w").write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    b = _lib.NucSeqs([path])
    try:
        r = fn(ctx, b, stat, rdm.SEP_LEN[stat], st, sz, **kw)
    finally:
        b.close()
    return (hexes(r["td"]) if stat == "td" else r["counts"].tolist()), r


@pytest.mark.parametrize("stat", ["gc", "cd", "td"])
def test_host_executor_equals_the_restatement_for_every_block_and_budget(tmp_path, stat):
    r = random.Random(31)
    seqs = random_genome(r, [700, 1, 333, 64, 0, 150])
    scaf = ref.scaffold(dict(enumerate(seqs)), stat)
    results = []
    for block in BLOCKS:
        st, sz = window_shapes(r, len(scaf), block)
        want = restated_windows(scaf, stat, st, sz)
        for budget in (0, 544 * 3):
            got, o = run_windows(emu.refdist, None, tmp_path, seqs, stat, st, sz, block=block, budget_bytes=budget)
            assert got == want
            assert o["batches"] == (-(-len(st) // 3) if stat == "td" and budget else 1) and o["bytes"] == len(scaf)
            if stat == "td":
                assert [int(x) for x in o["totals"][2:]] == tetra_counts(scaf)
            else:
                assert tuple(int(x) for x in o["totals"][:2]) == ref.gc_at(scaf)
    # the same windows for every block size: the same bytes
    st, sz = window_shapes(r, len(scaf), 64)
    for block in BLOCKS:
        results.append(run_windows(emu.refdist, None, tmp_path, seqs, stat, st, sz, block=block)[0])
    assert all(x == results[0] for x in results)


def test_run_writes_the_golden_files(host_executor, tmp_path):
    names = ["genes", "single"]
    paths, gffs = zip(*[write_case(tmp_path, CASES[n]) for n in names])
    for n in names:
        assert CASES[n]["numWindows"] and CASES[n]["results"]["gc"]["error"] is None
    R = rdm.ReferenceDistributions()
    for n, p, g in zip(names, paths, gffs):
        c = CASES[n]
        R.run([p], str(tmp_path / "out"), gffFiles=[g], numWindows=c["numWindows"], windowSizes=c["sizes"], seed=c["seed"])
        for stat, sub in (("gc", "deltaGC"), ("cd", "deltaCD"), ("td", "deltaTD")):
            assert open(str(tmp_path / "out" / sub / (n + ".tsv"))).read() == c["results"][stat]["file"]
    assert R.last_timing["drawn"] > 0 and set(R.last_timing) >= {"read", "scaffold", "copy_in", "blocks", "scan", "windows", "copy_out", "python"}


def test_bounds_files_equal_the_goldens_and_read_back(tmp_path):
    R = rdm.ReferenceDistributions()
    old = DefaultValues.DISTRIBUTION_DIR
    try:
        DefaultValues.DISTRIBUTION_DIR = str(tmp_path)
        g = GOLD["bounds"]
        (tmp_path / "gc").mkdir()
        for k, text in g["files"].items():
            open(str(tmp_path / "gc" / (k + ".tsv")), "w").write(text)
        open(str(tmp_path / "gc" / "notes.txt"), "w").write("not a genome\n")
        d = R.bounds(str(tmp_path / "gc"), str(tmp_path / "gc_dist.txt"), **g["params"])
        assert open(str(tmp_path / "gc_dist.txt")).read() == g["text"] == str(ref.bounds(g["files"], **g["params"]))
        assert common.readDistribution("gc_dist") == d and hexes(d.keys()) == g["centres"]
        assert all(type(k) is float and type(w) is int and type(p) is float and type(v) is float for k, a in d.items() for w, b in a.items() for p, v in b.items())
        g = GOLD["boundsTD"]
        (tmp_path / "td").mkdir()
        for k, text in g["files"].items():
            open(str(tmp_path / "td" / (k + ".tsv")), "w").write(text)
        d, bad = R.boundsTD(str(tmp_path / "td"), str(tmp_path / "td_dist.txt"), seed=g["seed"], maxPoints=g["cap"])
        want, wbad = ref.bounds_td(g["files"], g["seed"], cap=g["cap"])
        assert open(str(tmp_path / "td_dist.txt")).read() == g["text"] == str(want) and bad == g["bad"] == wbad == ["y"]
        assert common.readDistribution("td_dist") == d and sorted(d) == [500, 600, 700]
    finally:
        DefaultValues.DISTRIBUTION_DIR = old


def test_argument_refusals_need_no_device(tmp_path):
    ok = dict(stat=0, sep_len=0, block=0, scaffold_len=100, starts=[0, 90], sizes=[100, 10])
    _lib.refdist_check(**ok)
    for change in (dict(stat=3), dict(stat=-1), dict(sep_len=1025), dict(block=15), dict(block=(1 << 20) + 1), dict(sizes=[100, 11]), dict(sizes=[0, 10]), dict(starts=[-1, 90]),
                   dict(starts=[1, 90]), dict(scaffold_len=2 ** 31 - 1, starts=[], sizes=[])):
        with pytest.raises(_lib.CkmError) as e:
            _lib.refdist_check(**dict(ok, **change))
        assert e.value.code == (-7 if "scaffold_len" in change else -1)
    _lib.refdist_check(**dict(ok, scaffold_len=2 ** 31 - 2, block=16))
    R = rdm.ReferenceDistributions()
    p = str(tmp_path / "g.fna")
    open(p, "w").write(">a\nACGT\n")
    for bad in (0, -3, 1.5, True, "7"):
        with pytest.raises(ValueError):
            R.deltaGC(p, numWindows=bad)
        with pytest.raises(ValueError):
            R.deltaTD(p, numWindows=2, windowSizes=[4, bad])


def test_coding_lookups_equal_the_mask(tmp_path):
    from tests.seqwin_reference import coding_masks
    case = CASES["genes"]
    _, gff = write_case(tmp_path, case)
    mask = coding_masks(case["gff"])["genes"]
    r = random.Random(2)
    st = [r.randint(0, 400) for _ in range(300)] + [0, 0, 373, 374, 500]
    sz = [r.randint(1, 120) for _ in range(300)] + [1, 1000, 1, 1, 3]
    coding, total = _lib.refdist_coding(gff, "genes", st, sz)
    assert coding.tolist() == [int(np.sum(mask[s:s + w])) for s, w in zip(st, sz)] and total == int(np.sum(mask))
    coding, total = _lib.refdist_coding(gff, "stranger", st, sz)
    assert not coding.any() and total == 0
    with pytest.raises(_lib.CkmError):
        _lib.refdist_coding(str(tmp_path / "absent.gff"), "genes", st, sz)


def test_a_non_ascii_genome_is_computed_on_the_host(host_executor, tmp_path, caplog):
    seqs = {"a": "ACGTNACGGTéACGTTGCAAC", "b": "GGCATCGATT"}
    p = str(tmp_path / "uni.fna")
    open(p, "w", encoding="utf-8").write("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    R = rdm.ReferenceDistributions()
    with caplog.at_level(logging.DEBUG, logger="timestamp"):
        got = outcome(lambda: R.deltaGC(p, 6, [1, 5, 12], 9))
    assert got == outcome(lambda: ref.delta_gc(seqs, "uni", 6, [1, 5, 12], 9)) and R.last_timing["host"]
    assert any("non-ASCII" in m for m in caplog.messages)
    assert outcome(lambda: R.deltaTD(p, 6, [3, 5, 12], 9)) == outcome(lambda: ref.delta_td(seqs, "uni", 6, [3, 5, 12], 9))


def test_an_unsorted_size_list_fails_at_the_first_size_in_the_order_given(host_executor, tmp_path):
    seqs = {"a": "ACGTACGTACGTACGTACN" * 12}
    p, gff = str(tmp_path / "gaps.fna"), str(tmp_path / "gaps.gff")
    open(p, "w").write(">a\n%s\n" % seqs["a"])
    open(gff, "w").write("##gff-version  3\n")
    R = rdm.ReferenceDistributions()
    for sizes in ([60, 5, 30], [30, 60, 5], [5, 30, 60]):
        got = outcome(lambda: R.deltaCD(p, gff, 2, sizes, 4))
        assert got == outcome(lambda: ref.delta_cd(seqs, "##gff-version  3\n", "gaps", 2, sizes, 4))
        assert got["error"] == "ValueError" and "size %d " % next(w for w in sizes if w > 19) in got["message"]
    ok = outcome(lambda: R.deltaCD(p, gff, 2, [7, 5, 1000, 3], 4))
    assert ok == outcome(lambda: ref.delta_cd(seqs, "##gff-version  3\n", "gaps", 2, [7, 5, 1000, 3], 4)) and list(ok["dist"]) == ["7", "5"]


def test_the_numpy_restatement_of_td_equals_the_plain_one():
    r = random.Random(8)
    for lens in ([300, 0, 120], [5], [2, 1], []):
        seqs = dict(enumerate(random_genome(r, lens)))
        a, b = (outcome(lambda: f(seqs, "g", 7, [1, 3, 4, 5, 30, 100, 400], 2)) for f in (ref.delta_td, ref.delta_td_numpy))
        assert a == b
