#!/usr/bin/env python
"""Times SequenceWindows.tdWindows (the costliest of the four passes: base counts, 4-mers and the distance per window) over synthetic
bins on the device and prints one JSON line: the sums of last_timing over the bins.
usage: python tools/seqwin_bench.py --bins 64 --window 5000 [--mb-per-bin 4] [--contigs 40]"""
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
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--window", type=int, default=5000)
    ap.add_argument("--mb-per-bin", type=float, default=4.0)
    ap.add_argument("--contigs", type=int, default=40)
    a = ap.parse_args()
    from checkm_amd.seqWindows import SequenceWindows
    rng = np.random.default_rng(13)
    d = tempfile.mkdtemp(prefix="ckm_seqwin_bench_")
    n = int(a.mb_per_bin * (1 << 20)) // a.contigs
    paths, sigs = [], []
    for b in range(a.bins):
        paths.append(os.path.join(d, "bin%03d.fna" % b))
        with open(paths[-1], "w") as f:
            for c in range(a.contigs):
                f.write(">b%d_c%d\n%s\n" % (b, c, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes().decode()))
        rows = rng.random((a.contigs, 136))
        sigs.append({"b%d_c%d" % (b, c): rows[c] / rows[c].sum() for c in range(a.contigs)})
    s = SequenceWindows()
    s.tdWindows(paths[0], sigs[0], a.window)                  # first call: context, code objects
    total = {}
    t0 = time.perf_counter()
    for p, g in zip(paths, sigs):
        s.tdWindows(p, g, a.window)
        for k, v in s.last_timing.items():
            total[k] = total.get(k, 0) + v
    total.update(wall=time.perf_counter() - t0, bins=a.bins, window=a.window, megabytes=a.bins * a.mb_per_bin)
    print(json.dumps(total))


if __name__ == "__main__":
    main()
