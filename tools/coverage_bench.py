#!/usr/bin/env python
"""Times `checkm coverage` (checkm_amd.coverage.Coverage.run) on a synthetic sorted BAM file and prints one JSON line with the time split:
reading the bins, reading and inflating the BGZF blocks, the record offsets, copy in, the kernel, copy out, writing.  A warm-up call
first, then --reps timed calls; the median call is reported with the spread of the totals.

usage: python tools/coverage_bench.py --reads 2000000 [--refs 3000] [--reps 5]"""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from checkm_amd.coverage import Coverage
    from synthdata import bam as sbam
    d = tempfile.mkdtemp(prefix="ckm_coverage_bench_")
    # a block of records written once and repeated: the generator is plain Python
    unit = min(a.reads, 20000)
    refs, recs = sbam.synthetic(unit, min(a.refs, unit), seed=11)
    reps = max(1, a.reads // unit)
    refs = [("contig_%06d" % k, 5000) for k in range(len(refs) * reps)]
    body = []
    for k in range(reps):
        body.append(b"".join(sbam.record_bytes(dict(r, ref=r["ref"] + k * (len(refs) // reps))) for r in recs))
    path = os.path.join(d, "bench.bam")
    with open(path, "wb") as f:
        f.write(sbam.bgzf(sbam.header_bytes(refs) + b"".join(body)))
    open(path + ".bai", "wb").close()
    fa = os.path.join(d, "bin_1.fna")
    with open(fa, "w") as f:
        for name, n in refs[:len(refs) // 2]:
            f.write(">%s\n%s\n" % (name, "ACGT" * (n // 4)))
    out = os.path.join(d, "coverage.tsv")
    c = Coverage(1)
    null = open(os.devnull, "w")
    runs = []
    for k in range(a.reps + 1):
        old, sys.stdout = sys.stdout, null
        try:
            c.run([fa], [path], out, *sbam.PARAMS)
        finally:
            sys.stdout = old
        if k:
            runs.append(dict(c.last_timing))
    bam_bytes = os.path.getsize(path)
    shutil.rmtree(d, ignore_errors=True)
    runs.sort(key=lambda t: t["s_total"])
    med = runs[len(runs) // 2]
    totals = [t["s_total"] for t in runs]
    print(json.dumps(dict(what="Coverage.run on one synthetic sorted BAM, median of %d calls after a warm-up" % a.reps, reads=int(med["records"]), references=len(refs),
                          bam_bytes=bam_bytes, inflated_bytes=int(med["inflated_bytes"]), bgzf_blocks=int(med["blocks"]), batches=int(med["batches"]),
                          s_total=round(med["s_total"], 5), s_total_min=round(min(totals), 5), s_total_max=round(max(totals), 5), s_total_stdev=round(statistics.pstdev(totals), 5),
                          s_bins=round(med["s_bins"], 5), ms_read=round(med["ms_read"], 4), ms_inflate=round(med["ms_inflate"], 4), ms_offsets=round(med["ms_offsets"], 4),
                          ms_copy_in=round(med["ms_upload"], 4), ms_kernel=round(med["ms_kernel"], 4), ms_copy_out=round(med["ms_download"], 4),
                          ms_library_total=round(med["ms_total"], 4), s_write=round(med["s_write"], 5), reads_per_second=round(med["records"] / med["s_total"], 1))))


if __name__ == "__main__":
    main()
