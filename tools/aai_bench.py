#!/usr/bin/env python
"""Times AminoAcidIdentity.run over a synthetic storage/aai_qa tree on the device and prints one JSON line: last_timing (list, read,
pack, copy in, kernel, copy out, Python; groups, pairs, batches) with the wall time of `run`, and -- in the same process, on the same
tree -- the wall time of `_run_host`, the run with every pair on the host loop, which is what `run` was before the device pass.  Both
results are compared at ==.  The line is also written to profiles/r16_aai_bench_line.json.  Not part of bench.py.
usage: python tools/aai_bench.py --bins 64 --markers 20 --copies 12 [--big 300] [--columns 180]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_tree(d, bins, markers, copies, big=0, columns=180, seed=16):
    """<d>/bins/<bin>/ and <d>/storage/aai_qa/<bin>/<marker>.masked.faa: `bins` bins of `markers` markers with `copies` copies each, and,
    with big > 0, one more bin whose single marker has `big` copies.  A copy is its marker's consensus with a tenth of the columns
    redrawn, a twentieth gapped and gap runs of up to a fifth of the row at both ends.  Returns d."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    shape = [("bin%03d" % b, markers, copies) for b in range(bins)] + ([("big", 1, big)] if big else [])
    for binId, nm, nc in shape:
        os.makedirs(os.path.join(d, "bins", binId))
        folder = os.path.join(d, "storage", "aai_qa", binId)
        os.makedirs(folder)
        for m in range(nm):
            L = int(columns * (0.5 + rng.random()))
            consensus = rng.choice(letters, L)
            with open(os.path.join(folder, "PF%05d.%d.masked.faa" % (m, 1 + m % 20)), "w") as f:
                for c in range(nc):
                    row = consensus.copy()
                    redraw = rng.random(L) < 0.10
                    row[redraw] = rng.choice(letters, int(redraw.sum()))
                    row[rng.random(L) < 0.05] = ord("-")
                    row[:int(rng.integers(0, L // 5 + 1))] = ord("-")
                    row[L - int(rng.integers(0, L // 5 + 1)):] = ord("-")
                    f.write(">%s&&gene_%d_%d [e-value=1e-30,score=100.0]\n%s\n" % (binId, m, c, row.tobytes().decode()))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--markers", type=int, default=20)
    ap.add_argument("--copies", type=int, default=12)
    ap.add_argument("--big", type=int, default=300)
    ap.add_argument("--columns", type=int, default=180)
    a = ap.parse_args()
    from checkm_amd.aminoAcidIdentity import AminoAcidIdentity
    warm = synth_tree(tempfile.mkdtemp(prefix="ckm_aai_warm_"), 1, 1, 2)
    AminoAcidIdentity().run(0.9, warm, None)                     # first call: context, code objects
    d = synth_tree(tempfile.mkdtemp(prefix="ckm_aai_bench_"), a.bins, a.markers, a.copies, a.big, a.columns)
    dev, host = AminoAcidIdentity(), AminoAcidIdentity()
    AminoAcidIdentity()._run_host(0.9, d, os.path.join(d, "warm.txt"))          # the files are in the page cache for both timed runs
    t0 = time.perf_counter()
    dev.run(0.9, d, os.path.join(d, "device.txt"))
    t1 = time.perf_counter()
    host._run_host(0.9, d, os.path.join(d, "host.txt"))
    t2 = time.perf_counter()
    same = (dev.aaiRawScores == host.aaiRawScores and dev.aaiHetero == host.aaiHetero and dev.aaiMeanBinHetero == host.aaiMeanBinHetero and
            open(os.path.join(d, "device.txt"), "rb").read() == open(os.path.join(d, "host.txt"), "rb").read())
    out = dict(dev.last_timing, wall=t1 - t0, host_loop_wall=t2 - t1, results_equal=bool(same), bins=a.bins, markers=a.markers, copies=a.copies, big=a.big,
               columns=a.columns)
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "r16_aai_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
