#!/usr/bin/env python
"""Times Unbinned.run over a synthetic assembly on the device and prints one JSON line: the split of last_timing, and -- in the same
process, on the same batch read once by ckm_nucseq_read -- the GB/s of the count kernel of ckm_unbinned_count with every sequence kept
and of the count kernel of ckm_nucstats_run(tetra=0), the earlier way to these counts (both from HIP events around the kernel alone,
over the bytes each kernel reads; the median and the spread of the timed repeats after a warm-up).  The line is also written to
profiles/r15_unbinned_bench_line.json.  Not part of bench.py.
usage: python tools/unbinned_bench.py --bins 20 --mb 256 [--contig 5000] [--repeats 7] [--min-len 1000]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_assembly(d, bins, mb, contig, seed=15):
    """An assembly of about `mb` MiB in contigs of 200 .. 2 * contig bases (60 per line) and `bins` bin files that hold every second
    contig between them.  Returns (bin paths, assembly path)."""
    rng = np.random.default_rng(seed)
    total, k = int(mb * (1 << 20)), 0
    asm = os.path.join(d, "assembly.fna")
    outs = [open(os.path.join(d, "bin%03d.fna" % b), "w") for b in range(bins)]
    letters = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    with open(asm, "w") as f:
        while total > 0:
            n = int(rng.integers(200, 2 * contig))
            s = rng.choice(letters, n, p=[0.24, 0.24, 0.24, 0.24, 0.01, 0.01, 0.005, 0.005, 0.005, 0.005]).tobytes().decode()
            rec = ">contig_%d len=%d\n%s\n" % (k, n, "\n".join(s[i:i + 60] for i in range(0, n, 60)))
            f.write(rec)
            if bins and k % 2 == 0:
                outs[(k // 2) % bins].write(rec)
            total -= n
            k += 1
    for o in outs:
        o.close()
    return [o.name for o in outs], asm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--mb", type=float, default=256.0)
    ap.add_argument("--contig", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--min-len", type=int, default=1000)
    a = ap.parse_args()
    from checkm_amd import _lib, runtime
    from checkm_amd.unbinned import Unbinned
    d = tempfile.mkdtemp(prefix="ckm_unbinned_bench_")
    binFiles, asm = synth_assembly(d, a.bins, a.mb, a.contig)
    U = Unbinned()
    U.run(binFiles[:1], binFiles[0], os.path.join(d, "warm.fna"), os.path.join(d, "warm.tsv"), a.min_len)     # first call: context, code objects
    t0 = time.perf_counter()
    U.run(binFiles, asm, os.path.join(d, "unbinned.fna"), os.path.join(d, "unbinned.tsv"), a.min_len)
    out = dict(U.last_timing, wall=time.perf_counter() - t0, megabytes=a.mb, min_len=a.min_len)
    # the two count kernels on one resident batch, every sequence kept
    ctx = runtime.get_ctx()
    seqs = _lib.NucSeqs([asm])
    try:
        keep = np.ones(seqs.nseq, dtype=np.uint8)
        new, old, same = [], [], True
        for rep in range(a.repeats + 1):                        # alternating; the first pair is the warm-up
            r = _lib.unbinned_count(ctx, seqs, keep)
            s = _lib.nucstats(ctx, seqs, tetra=False)
            same = same and np.array_equal(r["counts"][:, :4], s["count"][:, :4]) and np.array_equal(r["counts"][:, 4], s["count"][:, 6])
            if rep:
                new.append(r["bytes"] / (r["ms_count"] * 1e6))
                old.append(s["bytes"] / (s["ms_count"] * 1e6))
        out.update(count_gbps=float(np.median(new)), count_gbps_min=min(new), count_gbps_max=max(new), nucstats_count_gbps=float(np.median(old)),
                   nucstats_count_gbps_min=min(old), nucstats_count_gbps_max=max(old), repeats=a.repeats, counts_equal=bool(same), count_bytes=int(r["bytes"]),
                   nucstats_bytes=int(s["bytes"]), count_batches=int(r["batches"]))
    finally:
        seqs.close()
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "r15_unbinned_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
