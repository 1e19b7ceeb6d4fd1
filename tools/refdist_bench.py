#!/usr/bin/env python
"""Times ReferenceDistributions.deltaTD (the costliest of the three samplings: 41 window sizes, the 4-mer counts and the distance of
every drawn window) over synthetic genomes on the device, prints one JSON line -- the sums of last_timing over the genomes and the
windows per second -- and writes it to profiles/r14_refdist_bench_line.json.  Not part of bench.py.
usage: python tools/refdist_bench.py --genomes 8 --mb 4 [--windows 10000] [--contigs 20] [--block 0]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--mb", type=float, default=4.0)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--contigs", type=int, default=20)
    ap.add_argument("--block", type=int, default=0)
    a = ap.parse_args()
    from checkm_amd.referenceDistributions import ReferenceDistributions
    rng = np.random.default_rng(14)
    d = tempfile.mkdtemp(prefix="ckm_refdist_bench_")
    n = int(a.mb * (1 << 20)) // a.contigs
    paths = []
    for g in range(a.genomes):
        paths.append(os.path.join(d, "genome%03d.fna" % g))
        with open(paths[-1], "w") as f:
            for c in range(a.contigs):
                f.write(">g%d_c%d\n%s\n" % (g, c, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes().decode()))
    R = ReferenceDistributions()
    R.block = a.block
    R.deltaTD(paths[0], 8, [500])                             # first call: context, code objects
    total = {}
    t0 = time.perf_counter()
    for p in paths:
        R.deltaTD(p, a.windows)
        for k, v in R.last_timing.items():
            if not isinstance(v, bool):
                total[k] = total.get(k, 0) + v
    wall = time.perf_counter() - t0
    total.update(wall=wall, genomes=a.genomes, megabytes=a.genomes * a.mb, windows_per_size=a.windows, block=a.block or 256, windows_per_second=total["drawn"] / wall,
                 windows_per_second_on_device=total["drawn"] / max(1e-9, total["blocks"] + total["scan"] + total["windows"]))
    line = json.dumps(total)
    with open(os.path.join(ROOT, "profiles", "r14_refdist_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
