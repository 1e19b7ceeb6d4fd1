#!/usr/bin/env python
"""Goldens of `checkm merge` produced by the REFERENCE's own Merger, ResultsParser and MarkerSet (checkm/merger.py imported read-only from
a CheckM source tree named by CHECKM_SOURCE).  Bins are row subsets of the tables of
tests/golden/reduce_cases.json (so the vetting, clan and adjacency filters run before the merge); only data is recorded: which rows
each bin keeps, extra rows, the marker set structures, thresholds, and the bytes of merger.tsv or the failure.  Here only.

usage: CHECKM_SOURCE=<checkm source> python tools/gen_merger_golden.py > tests/golden/merger_cases.json
       python tools/gen_merger_golden.py --time --bins 200 [--markers 104]      the reference's pair loop, pairs per second on one core"""
import argparse
import json
import logging
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = tempfile.mkdtemp(prefix="ckm_data_")          # the reference wants a data root at import time
os.makedirs(os.path.join(DATA, "pfam"))
open(os.path.join(DATA, "pfam", "Pfam-A.hmm.dat"), "w").close()
os.environ["CHECKM_DATA_PATH"] = DATA
sys.dont_write_bytecode = True

from tests import merger_common as mc  # noqa: E402

DEFAULT = [5.0, 10.0, 50.0, 20.0]


class Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.text = []

    def emit(self, record):
        self.text.append(record.getMessage())


def build_world(cases):
    """Ten bins over reduce case 50 (13 models, clans, 15 marker genes of which the table reaches 10), chosen gene by gene from the hits
    the full table keeps; ids whose sorted order is neither insertion nor numeric."""
    ci = 50
    case = cases[ci]
    lines = case["domtblout"].splitlines()
    rows = [k for k, ln in enumerate(lines) if ln and not ln.startswith("#")]
    kept = [(acc, [h[0] for h in hits if "&&" not in h[0]]) for acc, hits in case["runs"][0]["expected"]["markerHits"]]
    assert len(kept) == 10

    def pick(genes, copies=1):
        want = set((acc, t) for acc, targets in genes for t in targets[:copies])
        out = []
        for k in rows:
            tok = lines[k].split()
            if (tok[4] if tok[4] != "-" else tok[3], tok[0]) in want:
                out.append(k)
        return out
    model = next(ln for ln in lines if ln.split()[0:1] == ["NODE_2_length_32657_cov_12.62_30"] and "PF30488.1" in ln)
    extra = "".join("copy_%d_1 %s\n" % (k, model.split(" ", 1)[1]) for k in range(3))
    bins = [dict(id="bin10", rows=rows, extra=extra),                       # everything, and six copies of PF30488.1
            dict(id="bin2", rows=pick(kept[0:5]), extra=""),
            dict(id="Bin3", rows=pick(kept[5:10]), extra=""),               # complements bin2
            dict(id="b\u00edn4", rows=pick(kept[0:8]), extra=""),
            dict(id="bin1", rows=pick(kept[0:5], 3), extra=""),             # bin2 with every copy
            dict(id="a_nohits", rows=[], extra=""),
            dict(id="z_missing", rows=None, extra=""),                      # no table file at all
            dict(id="bin7", rows=pick(kept[2:9]), extra=""),
            dict(id="bin8", rows=pick(kept[0:6]), extra=""),
            dict(id="bin9", rows=pick(kept[4:10], 2), extra="")]
    a = [sorted(s) for s in case["marker_sets"]]
    b = a[:-1] + [a[-1] + [a[0][1]], [a[1][0], a[2][0]]]                    # the same genes, three more entries
    assert set(sum(a, [])) == set(sum(b, [])) and len(sum(b, [])) == len(sum(a, [])) + 3
    return dict(name="ten_bins", reduce_case=ci, bins=bins, structures=dict(A=a, B=b),
                assign={x["id"]: ("B" if k % 3 == 1 else "A") for k, x in enumerate(bins)})


def run_reference(world, cases, thr, cap, binmarkersets=None, models_for=None):
    from checkm.merger import Merger
    d = tempfile.mkdtemp(prefix="ckm_merger_gold_")
    models, bms = mc.materialise(world, cases, d, mc.reference_classes(), marker_sets=binmarkersets, models_for=models_for)
    del cap.text[:]
    try:
        path = Merger().run([], d, mc.TABLE, models, bms, *thr)
    except SystemExit as e:
        return dict(error=dict(type="SystemExit", code=e.code, log=list(cap.text)))
    except (ZeroDivisionError, IndexError, KeyError) as e:
        return dict(error=dict(type=type(e).__name__, args=[str(x) for x in e.args]))
    return dict(output=open(path, encoding="utf-8").read())


def pair_values(world, cases, pair):
    """compM, contM, deltaComp, deltaCont of one pair by the reference's own geneCounts."""
    from checkm.resultsParser import ResultsParser
    d = tempfile.mkdtemp(prefix="ckm_merger_gold_")
    models, bms = mc.materialise(world, cases, d, mc.reference_classes())
    rp = ResultsParser(models)
    rp.parseBinHits(d, mc.TABLE)
    I, J = pair
    ri, rj = rp.results[I], rp.results[J]
    gi = ri.geneCounts(bms[I].mostSpecificMarkerSet(), ri.markerHits, True)
    gj = rj.geneCounts(bms[J].mostSpecificMarkerSet(), rj.markerHits, True)
    merged = {m: list(h) for m, h in ri.markerHits.items()}
    for m, h in rj.markerHits.items():
        merged.setdefault(m, []).extend(h)
    gm = ri.geneCounts(bms[J].mostSpecificMarkerSet(), merged, True)
    assert max(len(h) for h in rp.results["bin10"].markerHits.values()) > 5
    return dict(compM=gm[6], contM=gm[7], deltaComp=gm[6] - max(gi[6], gj[6]), deltaCont=gm[7] - max(gi[7], gj[7]))


def golden():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "reduce_cases.json")))["cases"]
    cap = Capture()
    logging.getLogger("timestamp").addHandler(cap)
    world = build_world(cases)
    runs = []
    for thr in (DEFAULT, [0.0, 1000.0, 0.0, 1000.0], [-1000.0, 1000.0, -1000.0, 1000.0]):
        runs.append(dict(thr=thr, **run_reference(world, cases, thr, cap)))
    npairs = len(world["bins"]) * (len(world["bins"]) - 1) // 2
    lines = runs[2]["output"].splitlines()[1:]
    assert len(lines) == npairs and any("\t-" in ln for ln in lines)
    ndef = len(runs[0]["output"].splitlines()) - 1
    assert 0 < ndef < npairs, ndef
    # "J's set" is observable: a pair whose bins use different structures
    assert any(world["assign"][ln.split("\t")[0]] != world["assign"][ln.split("\t")[1]] for ln in lines)
    # thresholds exactly at a value that occurs: >= keeps the pair, < drops it
    pair = ("bin2", "bin7")          # (sorted order: bin2 < bin7)
    v = pair_values(world, cases, pair)
    loose = [-1000.0, 1000.0, -1000.0, 1000.0]
    for k, (name, kept) in enumerate((("deltaComp", True), ("deltaCont", False), ("compM", True), ("contM", False))):
        thr = list(loose)
        thr[k] = v[name]
        run = dict(thr=thr, thr_repr=[repr(x) for x in thr], exact=name, pair=list(pair), **run_reference(world, cases, thr, cap))
        has = any(ln.startswith("\t".join(pair) + "\t") for ln in run["output"].splitlines())
        assert has == kept, (name, has)
        assert len(run["output"].splitlines()) - 1 < npairs or kept
        runs.append(run)
    world["runs"] = runs
    # the failures
    fails = []
    ids = [b["id"] for b in world["bins"]]
    a = world["structures"]["A"]
    fails.append(dict(name="unequal_gene_sets", marker_sets={x: ([a[:-1]] if x == "bin8" else [a]) for x in ids}, thr=DEFAULT))
    fails.append(dict(name="empty_marker_set", marker_sets={x: [[]] for x in ids}, thr=DEFAULT))
    fails.append(dict(name="empty_input", marker_sets={}, thr=DEFAULT))
    fails.append(dict(name="bin_without_marker_sets", marker_sets={x: [a] for x in ids if x != "bin2"}, thr=DEFAULT))
    for f in fails:
        f.update(run_reference(world, cases, f["thr"], cap, binmarkersets=f["marker_sets"]))
    assert [f["error"]["type"] for f in fails] == ["SystemExit", "ZeroDivisionError", "IndexError", "KeyError"], fails
    world["failures"] = fails
    json.dump(dict(generator="tools/gen_merger_golden.py", reference="checkm/merger.py", worlds=[world]), sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")


def timing(nbins, nmarkers):
    """The reference's Merger.run with its parser replaced by prepared results: the pair loop alone, file writing included."""
    import checkm.merger as ref
    from checkm.markerSets import BinMarkerSets, MarkerSet
    from checkm.resultsParser import ResultsManager
    r = random.Random(7)
    genes = ["PF%05d.1" % k for k in range(nmarkers)]
    ms = MarkerSet(0, "k__Bacteria", 100, [set(genes[k:k + 3]) for k in range(0, nmarkers, 3)])
    results, bms = {}, {}
    for b in range(nbins):
        binId = "bin_%05d" % b
        rm = ResultsManager(binId, {})
        frac = r.uniform(0.2, 0.95)
        rm.markerHits = {g: [object()] * (2 if r.random() < 0.05 else 1) for g in genes if r.random() < frac}
        results[binId] = rm
        s = BinMarkerSets(binId, BinMarkerSets.TAXONOMIC_MARKER_SET)
        s.addMarkerSet(ms)
        bms[binId] = s

    class Prepared(object):
        def __init__(self, models):
            self.results = results

        def parseBinHits(self, outDir, hmmTableFile):
            pass
    ref.ResultsParser = Prepared
    d = tempfile.mkdtemp(prefix="ckm_merger_time_")
    t0 = time.perf_counter()
    ref.Merger().run([], d, "hmmer.analyze.txt", {}, bms, *DEFAULT)
    dt = time.perf_counter() - t0
    pairs = nbins * (nbins - 1) // 2
    print(json.dumps(dict(what="reference Merger.run pair loop (checkm/merger.py:64-108), one core", bins=nbins, markers=nmarkers, pairs=pairs, seconds=round(dt, 3),
                          pairs_per_second=round(pairs / dt, 1), reported=len(open(os.path.join(d, "merger.tsv")).read().splitlines()) - 1,
                          extrapolated_seconds_1000_bins=round(499500 / (pairs / dt), 1))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--markers", type=int, default=104)
    a = ap.parse_args()
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    if a.time:
        timing(a.bins, a.markers)
    else:
        golden()
