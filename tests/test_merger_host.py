"""`checkm merge` without a device: a numpy restatement of the reference's pair loop (checkm/merger.py:64-106) and a plain-Python writer,
pinned byte for byte to the files the reference's own Merger wrote (tests/golden/merger_cases.json, tools/gen_merger_golden.py); the
host executor of the kernels' source (checkm_amd/csrc/merge_dev.h, merge_host.h through tests/emu/merge_emu.cpp) against that
restatement; the argument refusals of ABI 10; the host C++ under ASan / UBSan; the drop-in binding."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import reduce_oracle as ro
from tests import merger_common as mc
from tests.emu import merge as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _world():
    world = json.load(open(os.path.join(GOLD, "merger_cases.json")))["worlds"][0]
    cases = json.load(open(os.path.join(GOLD, "reduce_cases.json")))["cases"]
    return world, cases


def _oracle_rows(world, cases):
    """The bins of a golden world reduced by the CPU oracle of the reduce half: (sorted ids, member, hit_sum, n_markers, genes)."""
    case = cases[world["reduce_case"]]
    models = {m["acc"]: m for m in case["models"]}
    sets = mc.world_marker_sets(world)
    hits = {}
    for b in world["bins"]:
        text = mc.bin_table(world, case, b)
        hits[b["id"]] = {} if text is None else ro.reduce_bin(text, models, case["pfam_dat"], sets[b["id"]][0])[0]
    genes = sorted(set(g for s in sets[world["bins"][0]["id"]][0] for g in s))
    ids, member, hit_sum, n_markers = mc.rows_from_hits(hits, sets, genes)
    return ids, member, hit_sum, n_markers, genes


def test_golden_world_is_what_the_issue_asks_for():
    world, _cases = _world()
    ids = [b["id"] for b in world["bins"]]
    assert 8 <= len(ids) <= 12 and sorted(ids) != ids and sorted(ids) != sorted(ids, key=lambda s: (len(s), s))
    assert any(ord(c) > 127 for x in ids for c in x) and {"bin10", "bin2", "Bin3"} <= set(ids)
    runs = world["runs"]
    assert [r["thr"] for r in runs[:3]] == [[5.0, 10.0, 50.0, 20.0], [0.0, 1000.0, 0.0, 1000.0], [-1000.0, 1000.0, -1000.0, 1000.0]]
    npairs = len(ids) * (len(ids) - 1) // 2
    assert 0 < len(runs[0]["output"].splitlines()) - 1 < npairs and len(runs[2]["output"].splitlines()) - 1 == npairs
    assert [r["exact"] for r in runs[3:]] == ["deltaComp", "deltaCont", "compM", "contM"]
    assert all([repr(x) for x in r["thr"]] == r["thr_repr"] for r in runs[3:])
    assert [f["error"]["type"] for f in world["failures"]] == ["SystemExit", "ZeroDivisionError", "IndexError", "KeyError"]
    assert os.path.getsize(os.path.join(GOLD, "merger_cases.json")) < 64 << 10


def test_restatement_and_writer_equal_the_reference_files():
    world, cases = _world()
    ids, member, hit_sum, n_markers, _genes = _oracle_rows(world, cases)
    assert len(set(n_markers.tolist())) == 2                    # two set structures: "J's set" is observable
    assert hit_sum.max() > member.sum(axis=1).max() and (member.sum(axis=1) == 0).sum() >= 2
    for run in world["runs"]:
        i, j, cols = mc.restate(member, hit_sum, n_markers, run["thr"])
        assert mc.HEADER + mc.write_lines(ids, i, j, cols) == run["output"], run["thr"]
    # swapping I and J changes a line: the pair is judged by J's marker set
    loose = world["runs"][2]["thr"]
    swap = np.arange(len(ids))[::-1]
    i, j, cols = mc.restate(member[swap], hit_sum[swap], n_markers[swap], loose)
    assert sorted(cols["comp_merged"].tolist()) != sorted(mc.restate(member, hit_sum, n_markers, loose)[2]["comp_merged"].tolist())


def test_host_executor_equals_the_reference_files():
    world, cases = _world()
    ids, member, hit_sum, n_markers, genes = _oracle_rows(world, cases)
    bits = mc.pack(member)
    for run in world["runs"]:
        for cap in (0, 1, 7):
            res = emu.merge_pairs(bits, hit_sum, n_markers, len(genes), run["thr"], cap_pairs=cap)
            assert (mc.HEADER.encode() + emu.lines([x.encode() for x in ids], res)).decode() == run["output"], (run["thr"], cap)


@pytest.mark.parametrize("ngenes", [40, 104, 150, 1050, 2500])          # 1, 2, 3, 17, 40 words
@pytest.mark.parametrize("nbins", [1, 2, 63, 64, 65, 257])
def test_host_executor_equals_the_restatement(nbins, ngenes):
    member, hit_sum, n_markers = mc.synthetic(nbins, ngenes, seed=nbins * 7919 + ngenes)
    if nbins > 2:
        member[1] = False; hit_sum[1] = 0                       # an all-zero row
        member[2] = True; hit_sum[2] = ngenes + 3               # an all-one row
    bits = mc.pack(member)
    assert bits.shape == (nbins, (ngenes + 63) // 64)
    ids = ["b%04d" % k for k in range(nbins)]
    for thr in ([5.0, 10.0, 50.0, 20.0], [-1000.0, 1000.0, -1000.0, 1000.0], [0.0, 30.0, 60.0, 40.0]):
        i, j, cols = mc.restate(member, hit_sum, n_markers, thr)
        want = mc.write_lines(ids, i, j, cols)
        results = [emu.merge_pairs(bits, hit_sum, n_markers, ngenes, thr)]
        if nbins <= 65 or ngenes == 104:
            results.append(emu.merge_pairs(bits, hit_sum, n_markers, ngenes, thr, cap_pairs=1, pass_rows=64))        # batches of one row, count passes of one tile
            assert results[1]["nbatches"] == len(set(i.tolist()))
        for res in results:
            assert res["npairs"] == len(i) and (res["i"] == i).all() and (res["j"] == j).all()
            for f in mc.COLUMNS:
                assert (res[f] == cols[f]).all(), (f, thr)
            assert emu.lines(ids, res).decode() == want
    if nbins > 1:
        assert len(mc.restate(member, hit_sum, n_markers, [-1000.0, 1000.0, -1000.0, 1000.0])[0]) == nbins * (nbins - 1) // 2


def test_pack_rows_layout():
    member = np.zeros((3, 130), dtype=bool)
    member[0, 0] = member[0, 63] = member[1, 64] = member[2, 129] = True
    bits = mc.pack(member)
    assert bits.dtype == np.uint64 and bits.shape == (3, 3)
    assert bits.tolist() == [[(1 << 63) | 1, 0, 0], [0, 1, 0], [0, 0, 2]]
    assert mc.pack(np.zeros((2, 0), dtype=bool)).shape == (2, 1)


def test_bin_rows_reads_unmaterialised_bins_from_the_kept_key_ids():
    """A bin whose hit dict nobody has built is counted from the key ids of its kept rows; the same bin as a dict gives the same row, and
    a key the reduction never saw stays absent."""
    from types import SimpleNamespace
    from checkm_amd import qa as cqa
    from checkm_amd.markerSets import BinMarkerSets, MarkerSet
    from checkm_amd.merger import bin_rows
    from checkm_amd.resultsParser import ResultsManager
    genes = ["g%02d" % k for k in range(70)]
    keys = cqa.KeyTable()
    for name in ["other_model"] + genes[:60]:
        keys.get(name)
    r = np.random.RandomState(5)
    kept = [r.randint(0, 61, size=n).astype(np.uint32) for n in (40, 0, 90)]
    res = SimpleNamespace(kept_bin_off=np.cumsum([0] + [len(k) for k in kept]), kept_key=np.concatenate(kept))
    ms = MarkerSet(0, "k__Bacteria", 10, [set(genes[:30]), set(genes[30:])])
    lazy, plain, bms = {}, {}, {}
    for b in range(3):
        binId = "bin%d" % b
        rm = ResultsManager(binId, {})
        rm._lazy = (res, b, keys, None)
        lazy[binId] = rm
        rp = ResultsManager(binId, {})
        d = {}
        for k in kept[b].tolist():
            d.setdefault(keys.names[k], []).append(None)
        rp.markerHits = d
        plain[binId] = rp
        s = BinMarkerSets(binId, BinMarkerSets.TAXONOMIC_MARKER_SET)
        s.addMarkerSet(ms)
        bms[binId] = s
    ids = sorted(lazy)
    a = bin_rows(lazy, ids, bms, sorted(genes))
    b = bin_rows(plain, ids, bms, sorted(genes))
    assert all(lazy[x]._lazy is not None for x in ids)                 # nothing was materialised
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    assert a[2].tolist() == [70, 70, 70] and a[0][1].sum() == 0 and a[1][1] == 0 and not a[0][:, 60:].any()
    assert a[1][0] == sum(1 for k in kept[0].tolist() if k != 0)        # hits to "other_model" are outside the gene set
    with pytest.raises(KeyError):
        bin_rows(plain, ids, {k: v for k, v in bms.items() if k != "bin1"}, sorted(genes))
    s = BinMarkerSets("bin2", BinMarkerSets.TAXONOMIC_MARKER_SET)
    s.addMarkerSet(MarkerSet(0, "k__Bacteria", 10, []))
    with pytest.raises(ZeroDivisionError, match="float division by zero"):
        bin_rows(plain, ids, dict(bms, bin2=s), sorted(genes))


def test_abi_10_refuses_bad_arguments_without_a_device():
    from checkm_amd import _lib
    lib = _lib.load()
    assert lib.ckm_abi_version() == 12 == _lib.ABI_VERSION
    member, hit_sum, n_markers = mc.synthetic(5, 104, seed=1)
    bits = mc.pack(member)
    thr = [5.0, 10.0, 50.0, 20.0]
    _lib.merge_check(bits, hit_sum, n_markers, 104, thr)
    assert emu.check(bits, hit_sum, n_markers, 104, thr) == ""
    bad = n_markers.copy(); bad[3] = 0
    with pytest.raises(_lib.CkmError) as e:
        _lib.merge_check(bits, hit_sum, bad, 104, thr)
    assert e.value.code == -1 and "n_markers" in str(e.value) and "n_markers" in emu.check(bits, hit_sum, bad, 104, thr)
    bad[3] = -4
    with pytest.raises(_lib.CkmError):
        _lib.merge_check(bits, hit_sum, bad, 104, thr)
    stray = bits.copy(); stray[2, 1] |= np.uint64(1 << 40)                 # gene 104 of 104
    with pytest.raises(_lib.CkmError) as e:
        _lib.merge_check(stray, hit_sum, n_markers, 104, thr)
    assert "beyond the gene count" in str(e.value)
    neg = hit_sum.copy(); neg[0] = -1
    with pytest.raises(_lib.CkmError):
        _lib.merge_check(bits, neg, n_markers, 104, thr)
    t = np.asarray(thr)
    args = (5, 104, bits.ctypes.data, hit_sum.ctypes.data, n_markers.ctypes.data)
    assert lib.ckm_merge_check(5, 0, *args[2:], t.ctypes.data) == -1
    assert lib.ckm_merge_check(*args, None) == -1 and lib.ckm_merge_check(5, 104, None, *args[3:], t.ctypes.data) == -1
    h = ctypes.c_void_p()
    assert lib.ckm_merge_run(None, *args, t.ctypes.data, None, None, 0, 1, ctypes.byref(h)) == -1 and not h.value       # no context: refused, not computed
    assert b"NULL" in lib.ckm_last_error()
    assert lib.ckm_merge_columns_get(None, None) == -1


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "merge_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "native", "merge_host_check.cpp"), os.path.join(ROOT, "tests", "emu", "merge_emu.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (run.stdout[-300:], run.stderr[-4000:])
    # with every pair reported and batches of one pair, every row but the last is a batch: sum of nbins - 1 over the harness's shapes
    assert json.loads(run.stdout.strip().split("\n")[0])["batches"] >= sum(n - 1 for n in (1, 2, 63, 64, 65, 130, 257))


def test_dropin_rebinds_merger_and_tolerates_its_absence(tmp_path):
    """A stand-in `checkm` package of its own, in a subprocess: with checkm/merger.py install() rebinds Merger; without it install() passes."""
    gold = json.load(open(os.path.join(GOLD, "reference_module_classes.json")))["classes"]
    for with_merger in (True, False):
        pkg = tmp_path / ("stand_in_%d" % with_merger) / "checkm"
        pkg.mkdir(parents=True)
        (pkg / "__init__.py").write_text("")
        for mod, classes in gold.items():
            (pkg / (mod.split(".")[1] + ".py")).write_text("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
        if with_merger:
            (pkg / "merger.py").write_text("class Merger(object):\n    pass\n")
        code = ("import checkm_amd.dropin as d; d.install()\n"
                "import importlib\n"
                "try:\n"
                "    m = importlib.import_module('checkm.merger')\n"
                "except ImportError:\n"
                "    print('absent')\n"
                "else:\n"
                "    import inspect\n"
                "    assert m.Merger.__module__ == 'checkm_amd.merger', m.Merger.__module__\n"
                "    assert list(inspect.signature(m.Merger.run).parameters) == ['self', 'binFiles', 'outDir', 'hmmTableFile', 'binIdToModels', 'binIdToBinMarkerSets',\n"
                "                                                               'minDeltaComp', 'maxDeltaCont', 'minMergedComp', 'maxMergedCont']\n"
                "    print('rebound')\n")
        env = dict(os.environ, PYTHONPATH=str(pkg.parent) + os.pathsep + ROOT, CHECKM_DATA_PATH=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == ("rebound" if with_merger else "absent"), (out.stdout, out.stderr[-1500:])
