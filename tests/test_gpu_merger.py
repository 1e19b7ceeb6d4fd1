"""GPU parity of `checkm merge`: Merger.run against the files the reference's own Merger wrote (tests/golden/merger_cases.json), and the
device comparison (ckm_merge_run) against the numpy restatement of the reference's pair loop at real sizes.
Bar: identical bytes of merger.tsv, identical failures, the nine float64 columns equal with ==."""
import hashlib
import json
import logging
import os

import numpy as np
import pytest

from checkm_amd import _lib
from tests import merger_common as mc
from tests.emu import merge as emu

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT = [5.0, 10.0, 50.0, 20.0]
LOOSE = [-1000.0, 1000.0, -1000.0, 1000.0]


def _world():
    world = json.load(open(os.path.join(GOLD, "merger_cases.json")))["worlds"][0]
    cases = json.load(open(os.path.join(GOLD, "reduce_cases.json")))["cases"]
    return world, cases


def test_merger_run_matches_reference_goldens(gpu_ctx, tmp_path, caplog):
    from checkm_amd.merger import Merger
    world, cases = _world()
    for k, run in enumerate(world["runs"]):
        d = str(tmp_path / ("run%d" % k))
        os.makedirs(d)
        models, bms = mc.materialise(world, cases, d, mc.package_classes())
        with caplog.at_level(logging.INFO, logger="timestamp"):
            caplog.clear()
            path = Merger().run([], d, mc.TABLE, models, bms, *run["thr"])
        assert path == os.path.join(d, "merger.tsv")
        assert open(path, encoding="utf-8").read() == run["output"], run["thr"]
        assert "Comparing marker sets between all pairs of bins." in [r.getMessage() for r in caplog.records]
    for f in world["failures"]:
        d = str(tmp_path / f["name"])
        os.makedirs(d)
        models, bms = mc.materialise(world, cases, d, mc.package_classes(), marker_sets=f["marker_sets"])
        err = f["error"]
        with caplog.at_level(logging.INFO, logger="timestamp"):
            caplog.clear()
            with pytest.raises(BaseException) as e:
                Merger().run([], d, mc.TABLE, models, bms, *f["thr"])
        assert type(e.value).__name__ == err["type"], f["name"]
        if err["type"] == "SystemExit":
            assert e.value.code == err["code"] and [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR] == err["log"]
        else:
            assert [str(a) for a in e.value.args] == err["args"], f["name"]
    with pytest.raises(SystemExit):
        Merger().run([], str(tmp_path / "no_such_dir"), mc.TABLE, {}, {}, *DEFAULT)


def test_merger_after_a_caller_edited_a_hit_dict(gpu_ctx, tmp_path):
    """A bin whose markerHits somebody has looked at and changed is read from the dict: an added key with an empty list is a member."""
    from checkm_amd.merger import Merger
    from checkm_amd.resultsParser import ResultsParser
    world, cases = _world()
    d = str(tmp_path / "w")
    os.makedirs(d)
    models, bms = mc.materialise(world, cases, d, mc.package_classes())
    rp = ResultsParser(models)
    rp.parseBinHits(d, mc.TABLE)
    genes = sorted(bms["bin2"].mostSpecificMarkerSet().getMarkerGenes())
    hits = rp.results["bin2"].markerHits
    absent = [g for g in genes if g not in hits]
    hits[absent[0]] = []
    out = str(tmp_path / "edited.tsv")
    assert Merger().compare(rp.results, bms, set(genes), out, *LOOSE) == out
    sets = mc.world_marker_sets(world)
    ids, member, hit_sum, n_markers = mc.rows_from_hits({b: dict(rp.results[b].markerHits) for b in rp.results}, sets, genes)
    assert member[ids.index("bin2"), genes.index(absent[0])]
    i, j, cols = mc.restate(member, hit_sum, n_markers, LOOSE)
    got = open(out, encoding="utf-8").read()
    assert got == mc.HEADER + mc.write_lines(ids, i, j, cols)
    assert got != world["runs"][2]["output"]


@pytest.mark.parametrize("nbins,ngenes,lo", [(3000, 104, 0.36), (1500, 2500, 0.3)])
def test_device_comparison_equals_the_restatement(gpu_ctx, tmp_path, nbins, ngenes, lo):
    """With the default thresholds the numpy restatement reports 3868 of 4 498 500 pairs at 3000 x 104 (0.086 %) and 205 of 1 124 250 at
    1500 x 2500 (0.018 %): the predicate removes all but a sliver.  The test asserts that the device reports the same pairs and prints
    the share and the kernel times it saw."""
    member, hit_sum, n_markers = mc.synthetic(nbins, ngenes, seed=11, lo=lo, hi=0.99, dup=0.01)
    bits = mc.pack(member)
    ids = ["bin_%05d" % k for k in range(nbins)]
    for thr in (DEFAULT, [0.0, 25.0, 55.0, 35.0]):
        i, j, cols = mc.restate(member, hit_sum, n_markers, thr)
        files = []
        for rep in range(2):
            path = str(tmp_path / ("m%d.tsv" % rep))
            with open(path, "w") as f:
                f.write(mc.HEADER)
            res = _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, ngenes, thr, bin_ids=ids, append_path=path)
            files.append(open(path, "rb").read())
        print("merge %d x %d thr %s: %d of %d pairs reported (%.4f %%), count %.3f ms, scan %.3f ms, fill %.3f ms" %
              (nbins, ngenes, thr, res["npairs"], res["compared"], 100.0 * res["npairs"] / res["compared"], res["ms_count"], res["ms_scan"], res["ms_fill"]))
        assert res["compared"] == nbins * (nbins - 1) // 2 and res["npairs"] == len(i)
        assert (res["i"] == i).all() and (res["j"] == j).all()
        for f in mc.COLUMNS:
            assert (res[f] == cols[f]).all(), f
        assert files[0] == files[1]                                   # two runs in one process: identical bytes
        assert files[0].decode() == mc.HEADER + mc.write_lines(ids, i, j, cols)
        if thr is DEFAULT:
            assert 5 <= len(i) <= 5000


def test_output_batches_do_not_change_the_file(gpu_ctx, tmp_path):
    """3000 bins with every pair reported (4 498 500 lines): under an output budget of 32 MB (a dozen batches) the file has the SHA-256
    of the file written in one batch, and the first and last rows are the restatement's."""
    nbins, ngenes = 3000, 104
    member, hit_sum, n_markers = mc.synthetic(nbins, ngenes, seed=11, lo=0.36, hi=0.99, dup=0.01)
    bits = mc.pack(member)
    ids = ["bin_%05d" % k for k in range(nbins)]
    digests, batches = [], []
    for name, budget in (("one", 1 << 30), ("many", 32 << 20)):
        path = str(tmp_path / (name + ".tsv"))
        res = _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, ngenes, LOOSE, bin_ids=ids, append_path=path, budget_bytes=budget, keep_columns=False)
        assert res["npairs"] == nbins * (nbins - 1) // 2 and "i" not in res
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        digests.append(h.hexdigest()); batches.append(res["nbatches"])
        if name == "many":
            with open(path, "rb") as f:
                head = f.read(4096).decode().splitlines()[:3]
                f.seek(-4096, os.SEEK_END)
                tail = f.read().decode().splitlines()[-2:]
        os.remove(path)
    assert batches[0] == 1 and batches[1] >= 10, batches
    assert digests[0] == digests[1]
    i, j, cols = mc.restate(member[:40], hit_sum[:40], n_markers[:40], LOOSE)
    assert head == mc.write_lines(ids, i, j, cols).splitlines()[:3]
    i, j, cols = mc.restate(member[-3:], hit_sum[-3:], n_markers[-3:], LOOSE)
    assert tail == mc.write_lines(ids[-3:], i, j, cols).splitlines()[-2:]


def test_small_shapes_and_batches_equal_the_host_executor(gpu_ctx):
    """The placement edges of the fill pass: fewer bins than a tile, exactly one, one more, three tile columns with a ragged last one;
    bit rows of one word, of one word and a bit, past one staged chunk of sixteen.  Every pair reported, and thresholds under which rows
    without a reported pair exist.  Output budgets of the default, of one 80-byte pair (every reporting row is a batch of its own) and of a
    hundred pairs, against the host executor of the kernels' source with the same batch caps: the pairs, their order, the nine columns and
    the number of batches are equal with ==."""
    some = [0.0, 25.0, 55.0, 35.0]
    for nbins in (2, 64, 65, 129, 200):
        for ngenes in (1, 64, 65, 1030):
            member, hit_sum, n_markers = mc.synthetic(nbins, ngenes, seed=11, lo=0.36, hi=0.99, dup=0.01)
            bits = mc.pack(member)
            for thr in (LOOSE, some):
                seen = {}
                for budget, cap in ((0, 0), (80, 1), (8000, 100)):
                    want = emu.merge_pairs(bits, hit_sum, n_markers, ngenes, thr, cap_pairs=cap)
                    res = _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, ngenes, thr, budget_bytes=budget)
                    where = (nbins, ngenes, thr, budget)
                    assert res["npairs"] == want["npairs"] and res["nbatches"] == want["nbatches"], where
                    assert (res["i"] == want["i"]).all() and (res["j"] == want["j"]).all(), where
                    for f in mc.COLUMNS:
                        assert (res[f] == want[f]).all(), (where, f)
                    seen[budget] = (want["npairs"], want["nbatches"])
                # the inputs are the ones the edges need: these figures are the host executor's
                if thr is LOOSE:
                    assert seen[0] == (nbins * (nbins - 1) // 2, 1)
                    if nbins == 65:
                        assert seen[80] == (2080, 64) and seen[8000] == (2080, 29)
                    if nbins == 200:
                        assert seen[80] == (19900, 199) and seen[8000] == (19900, 164)
                elif nbins >= 64:
                    assert 263 <= seen[0][0] <= 6643 and 27 <= seen[80][1] <= 197 and 3 <= seen[8000][1] <= 80, (where, seen)
                    assert seen[80][1] < nbins - 1, (where, seen)          # rows without a reported pair exist: they open no batch


def test_merge_pairs_refuses_bad_arguments_on_the_device(gpu_ctx):
    member, hit_sum, n_markers = mc.synthetic(70, 104, seed=3)
    bits = mc.pack(member)
    bad = n_markers.copy(); bad[69] = 0
    with pytest.raises(_lib.CkmError):
        _lib.merge_pairs(gpu_ctx, bits, hit_sum, bad, 104, DEFAULT)
    assert _lib.merge_pairs(gpu_ctx, bits[:1], hit_sum[:1], n_markers[:1], 104, LOOSE)["npairs"] == 0
    assert _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, 104, LOOSE)["npairs"] == 70 * 69 // 2
