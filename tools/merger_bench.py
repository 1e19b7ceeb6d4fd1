#!/usr/bin/env python
"""Times the comparison step of `checkm merge` (checkm_amd.merger.Merger.compare: everything of Merger.run after parseBinHits) on
synthetic bins and prints one JSON line with the time split: building the bit rows, copy in, the per-bin kernel, count kernel, scan,
fill kernel, copy out, formatting and writing.  A warm-up call first, then --reps timed calls; the median call is reported with the
spread of the totals.

usage: python tools/merger_bench.py --bins 1000 [--markers 104] [--reps 5] [--loose]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, required=True)
    ap.add_argument("--markers", type=int, default=104)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loose", action="store_true", help="thresholds that report every pair")
    a = ap.parse_args()
    from checkm_amd.markerSets import BinMarkerSets, MarkerSet
    from checkm_amd.merger import Merger
    from checkm_amd.resultsParser import ResultsManager
    r = np.random.RandomState(7)
    genes = ["PF%05d.1" % k for k in range(a.markers)]
    ms = MarkerSet(0, "k__Bacteria", 100, [set(genes[k:k + 3]) for k in range(0, a.markers, 3)])
    results, bms = {}, {}
    for b in range(a.bins):
        binId = "bin_%05d" % b
        rm = ResultsManager(binId, {})
        frac = r.uniform(0.2, 0.95)
        rm.markerHits = {g: [None] * (2 if r.random_sample() < 0.05 else 1) for g in genes if r.random_sample() < frac}
        results[binId] = rm
        s = BinMarkerSets(binId, BinMarkerSets.TAXONOMIC_MARKER_SET)
        s.addMarkerSet(ms)
        bms[binId] = s
    thr = (-1000.0, 1000.0, -1000.0, 1000.0) if a.loose else (5.0, 10.0, 50.0, 20.0)
    out = os.path.join(tempfile.mkdtemp(prefix="ckm_merger_bench_"), "merger.tsv")
    m = Merger()
    m.compare(results, bms, set(genes), out, *thr)          # warm-up: context, allocations
    runs = []
    for _ in range(a.reps):
        m.compare(results, bms, set(genes), out, *thr)
        runs.append(dict(m.last_timing))
    runs.sort(key=lambda t: t["s_total"])
    med = runs[len(runs) // 2]
    totals = [t["s_total"] for t in runs]
    print(json.dumps(dict(what="Merger.compare (Merger.run without parseBinHits), median of %d calls after a warm-up" % a.reps, bins=a.bins, markers=a.markers,
                          thresholds=list(thr), pairs=med["compared"], reported=med["npairs"], batches=med["nbatches"],
                          s_total=round(med["s_total"], 5), s_total_min=round(min(totals), 5), s_total_max=round(max(totals), 5),
                          s_total_stdev=round(statistics.pstdev(totals), 5),
                          s_bit_rows=round(med["s_rows"], 5), ms_copy_in=round(med["ms_upload"], 4), ms_bins_kernel=round(med["ms_bins"], 4),
                          ms_count_kernel=round(med["ms_count"], 4), ms_scan=round(med["ms_scan"], 4), ms_fill_kernel=round(med["ms_fill"], 4),
                          ms_copy_out=round(med["ms_download"], 4), ms_format_write=round(med["ms_write"], 4), ms_library_total=round(med["ms_total"], 4),
                          pairs_per_second=round(med["compared"] / med["s_total"], 1))))


if __name__ == "__main__":
    main()
