#!/usr/bin/env python
"""Times SSU_Finder.run on a synthetic assembly: one JSON line with the split of the run (read, tables, copy in, scan, compaction, copy
out, host hits, Python, write) and the cells (bases x strands x nodes) per second of the scan.  The data directory holds three seeded
models of 1533, 1478 and 1851 nodes (tests/ssufinder_synth.py), the assembly random contigs of 100 kb with --genes mutated copies of
the models' consensus planted on either strand.
usage: python tools/ssufinder_bench.py --mb 64 --genes 20 [--batch-mb N] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTIG = 100000
NODES = (1533, 1478, 1851)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--genes", type=int, default=20)
    ap.add_argument("--batch-mb", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    from checkm_amd import _lib, runtime
    from checkm_amd import ssuFinder as sf
    from checkm_amd.defaultValues import DefaultValues
    from tests import ssufinder_synth as syn
    rng = np.random.default_rng(a.seed)
    with tempfile.TemporaryDirectory() as d:
        cons = syn.data_dir(d, NODES, a.seed + 10)
        DefaultValues.CHECKM_DATA_DIR = d
        ncontigs = max(1, (a.mb << 20) // CONTIG)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        planted = defaultdict(list)
        for g in range(a.genes):
            planted[int(rng.integers(ncontigs))].append(g)
        contigs = os.path.join(d, "assembly.fna")
        with open(contigs, "wb") as f:
            for k in range(ncontigs):
                s = letters[rng.integers(0, 4, CONTIG)]
                for n, g in enumerate(planted.get(k, [])[:20]):
                    copy = syn.mutated_copy(rng, cons[("bacteria", "archaea", "euk")[g % 3]])
                    copy = syn.revcomp(copy) if g % 2 else copy
                    s[5000 * n + 100:5000 * n + 100 + len(copy)] = np.frombuffer(copy.encode(), dtype=np.uint8)
                f.write(b">contig%06d\n" % k + s.tobytes() + b"\n")
        ctx = runtime.get_ctx()
        acc = defaultdict(float)
        counts = defaultdict(int)

        def engine(tables, seqs, budget_bytes=0):
            t0 = time.perf_counter()
            res = _lib.nhmm_run(ctx, tables, seqs, a.batch_mb << 20)
            acc["call"] += time.perf_counter() - t0
            for f in _lib._NHMM_MS:
                acc[f] += res[f] / 1e3
            for f in ("tiles", "launches", "cells", "batches"):
                counts[f] += res[f]
            counts["rows"] += len(res["row_pos"])
            counts["hits"] += len(res["hit_from"])
            return res
        sf._nhmm_run = engine
        read_nucseqs = _lib.NucSeqs

        def timed_read(paths):
            t0 = time.perf_counter()
            s = read_nucseqs(paths)
            acc["read"] += time.perf_counter() - t0
            return s
        _lib.NucSeqs = timed_read
        finder = sf.SSU_Finder(1)
        post = finder._postProcess

        def timed_post(*args):
            t0 = time.perf_counter()
            post(*args)
            acc["write"] += time.perf_counter() - t0
        finder._postProcess = timed_post
        out = os.path.join(d, "out")
        t0 = time.perf_counter()
        finder.run(contigs, [], out, 1e-5, 200)
        total = time.perf_counter() - t0
        genes = len(open(os.path.join(out, "ssu_summary.tsv")).read().splitlines()) - 1
    line = dict(tool="ssufinder_bench", mb=a.mb, contigs=ncontigs, genes_planted=a.genes, genes_reported=genes, nodes=list(NODES), stride=sf.STRIDE,
                tiles=counts["tiles"], launches=counts["launches"], batches=counts["batches"], rows_reported=counts["rows"], hits=counts["hits"],
                seconds=dict(total=total, read=acc["read"], tables=acc["ms_tables"], copy_in=acc["ms_upload"], scan=acc["ms_scan"], compaction=acc["ms_compact"],
                             copy_out=acc["ms_download"], host_hits=acc["ms_hits"], python=total - acc["read"] - acc["call"] - acc["write"], write=acc["write"]),
                cells=counts["cells"], cells_per_second=counts["cells"] / acc["ms_scan"] if acc["ms_scan"] else None)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
