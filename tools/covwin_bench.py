#!/usr/bin/env python
"""Times CoverageWindows.run (checkm_amd.coverageWindows; `checkm gc_bias_plot`) on a synthetic sorted BAM file and prints one JSON line
with the time split: reading and inflating the BGZF blocks, the record offsets, copy in, the kernel, the scan, copy out, and Python
(the divisions and the dict).  A warm-up call first, then --reps timed calls; the median call is reported with the spread of the
totals.  The kernel time of ckm_coverage_run (`checkm coverage`) on the same file is put beside it, for scale.

usage: python tools/covwin_bench.py --reads 2000000 [--refs 3000] [--window 5000] [--reps 5]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, required=True)
    ap.add_argument("--refs", type=int, default=3000)
    ap.add_argument("--window", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from checkm_amd import _lib, runtime
    from checkm_amd.coverageWindows import CoverageWindows
    from synthdata import bam as sbam
    from tests import covwin_reference as wr
    d = tempfile.mkdtemp(prefix="ckm_covwin_bench_")
    # a block of records written once and repeated on further references: the generator is plain Python
    unit = min(a.reads, 20000)
    per = max(1, min(a.refs, unit))
    refs, recs = wr.synthetic(unit, per, seed=11, w=a.window, ref_len=lambda k: 20000 + 371 * (k % 97))
    reps = max(1, a.reads // unit)
    refs = [("contig_%06d" % k, refs[k % per][1]) for k in range(per * reps)]
    body = [b"".join(sbam.record_bytes(dict(r, ref=r["ref"] + k * per)) for r in recs) for k in range(reps)]
    path = os.path.join(d, "bench.bam")
    with open(path, "wb") as f:
        f.write(sbam.bgzf(sbam.header_bytes(refs) + b"".join(body)))
    open(path + ".bai", "wb").close()
    c = CoverageWindows(1)
    null = open(os.devnull, "w")
    runs = []
    for k in range(a.reps + 1):
        old, sys.stdout = sys.stdout, null
        try:
            c.run([], path, False, 0.98, 0.02, a.window)
        finally:
            sys.stdout = old
        if k:
            runs.append(dict(c.last_timing))
    b = _lib.Bam(path)
    try:
        _cnt, plain = _lib.coverage_counters(runtime.get_ctx(), b, *sbam.PARAMS)
    finally:
        b.close()
    bam_bytes = os.path.getsize(path)
    shutil.rmtree(d, ignore_errors=True)
    runs.sort(key=lambda t: t["s_total"])
    med = runs[len(runs) // 2]
    totals = [t["s_total"] for t in runs]
    print(json.dumps(dict(what="CoverageWindows.run on one synthetic sorted BAM, median of %d calls after a warm-up" % a.reps, reads=int(med["records"]), references=len(refs),
                          window=a.window, slots=int(med["slots"]), bam_bytes=bam_bytes, inflated_bytes=int(med["inflated_bytes"]), bgzf_blocks=int(med["blocks"]),
                          batches=int(med["batches"]), s_total=round(med["s_total"], 5), s_total_min=round(min(totals), 5), s_total_max=round(max(totals), 5),
                          s_total_stdev=round(statistics.pstdev(totals), 5), ms_read=round(med["ms_read"], 4), ms_inflate=round(med["ms_inflate"], 4),
                          ms_offsets=round(med["ms_offsets"], 4), ms_copy_in=round(med["ms_upload"], 4), ms_kernel=round(med["ms_kernel"], 4), ms_scan=round(med["ms_scan"], 4),
                          ms_copy_out=round(med["ms_download"], 4), ms_library_total=round(med["ms_total"], 4), s_python=round(med["s_python"], 5),
                          reads_per_second=round(med["records"] / med["s_total"], 1), ms_kernel_of_checkm_coverage_on_the_same_file=round(plain["ms_kernel"], 4))))


if __name__ == "__main__":
    main()
