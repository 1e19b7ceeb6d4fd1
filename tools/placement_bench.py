#!/usr/bin/env python
"""Times PplacerRunner.place on a synthetic reference package: one JSON line with the split of the call (read, eigen and tables, copy in,
matrices, sweeps, edge tables, scan, best edges, refine, copy out, tree and jplace) and the (query, edge, site) products per second of
the scan.  The package is a random tree whose leaves carry sequences mutated down the edges (a share 1 - exp(-length) of the sites redrawn
per edge), the model a seeded random reversible one, the queries copies of leaves with a twentieth of the sites redrawn and a third gapped.
usage: python tools/placement_bench.py --leaves 5656 --sites 6988 --queries 1000 --rates 4 [--batch-mb N] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LETTERS = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def synth_package(d, leaves, sites, seed):
    """A reference package directory under d: CONTENTS.json, the tree, the aligned FASTA, the model as a PAML .dat.  Returns the model's path."""
    from checkm_amd.pplacer import nodes_of, parse_newick, plain_name
    rng = np.random.default_rng(seed)
    parts = ["g%d" % k for k in range(leaves)]
    while len(parts) > 3:
        i, j = sorted(rng.choice(len(parts), size=2, replace=False).tolist())
        b, a = parts.pop(j), parts.pop(i)
        parts.append("(%s:%.5f,%s:%.5f)" % (a, rng.uniform(0.01, 0.3), b, rng.uniform(0.01, 0.3)))
    text = "(" + ",".join("%s:%.5f" % (p, rng.uniform(0.01, 0.3)) for p in parts) + ");"
    root = parse_newick(text)
    seqs = {root.num: LETTERS[rng.integers(0, 20, size=sites)]}
    fasta = []
    for v in reversed(nodes_of(root)):                             # parents before children
        if v.parent is not None:
            s = seqs[v.parent.num].copy()
            hit = rng.random(sites) < 1.0 - np.exp(-float(v.length))
            s[hit] = LETTERS[rng.integers(0, 20, size=int(hit.sum()))]
            seqs[v.num] = s
        if not v.children:
            fasta.append(">%s\n%s\n" % (plain_name(v.name), seqs.pop(v.num).tobytes().decode()))
    open(os.path.join(d, "tree.nwk"), "w").write(text + "\n")
    open(os.path.join(d, "ref.fasta"), "w").write("".join(fasta))
    json.dump({"files": {"tree": "tree.nwk", "aln_fasta": "ref.fasta"}}, open(os.path.join(d, "CONTENTS.json"), "w"))
    S = rng.gamma(1.0, 1.0, size=(20, 20)) + 0.05
    pi = rng.dirichlet(np.full(20, 5.0))
    with open(os.path.join(d, "model.dat"), "w") as f:
        for i in range(1, 20):
            f.write(" ".join(repr(float(S[i, j])) for j in range(i)) + "\n")
        f.write("\n" + " ".join(repr(float(x)) for x in pi) + "\n")
    return os.path.join(d, "model.dat")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=5656)
    ap.add_argument("--sites", type=int, default=6988)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--rates", type=int, default=4)
    ap.add_argument("--batch-mb", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    from checkm_amd import _lib, runtime
    from checkm_amd.pplacer import PplacerRunner, RefPkg, discrete_gamma, read_fasta
    rates, weights = discrete_gamma(0.7, a.rates) if a.rates > 1 else ((1.0,), (1.0,))
    with tempfile.TemporaryDirectory() as d:
        model = synth_package(d, a.leaves, a.sites, a.seed)
        t0 = time.perf_counter()
        ref = RefPkg.from_dir(d, model, rates, weights)
        read = time.perf_counter() - t0
        rng = np.random.default_rng(a.seed + 1)
        names = sorted(read_fasta(os.path.join(d, "ref.fasta")))
        queries = {}
        for k in range(a.queries):
            s = np.frombuffer(ref.alignment[names[int(rng.integers(len(names)))]].encode(), dtype=np.uint8).copy()
            hit = rng.random(a.sites) < 0.05
            s[hit] = LETTERS[rng.integers(0, 20, size=int(hit.sum()))]
            s[rng.random(a.sites) < 0.33] = ord("-")
            queries["bin%05d" % k] = s.tobytes().decode()
        runner = PplacerRunner(1)
        ctx = runtime.get_ctx()
        t0 = time.perf_counter()
        tables = runner._tables(ref, queries)
        eigen_tables = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = _lib.place_run(ctx, tables, a.batch_mb << 20)
        call = time.perf_counter() - t0
        t0 = time.perf_counter()
        placements = runner._placements(tables, res)
        ratios = time.perf_counter() - t0
        t0 = time.perf_counter()
        runner.writeJplace(ref, placements, os.path.join(d, "out.jplace"))
        open(os.path.join(d, "out.tre"), "w").write(runner.tog(ref, placements) + "\n")
        tree_jplace = time.perf_counter() - t0
    edges = tables.nnodes - 1
    ms = lambda f: res[f] / 1e3
    products = a.queries * edges * a.sites
    line = dict(tool="placement_bench", leaves=a.leaves, edges=edges, sites=a.sites, queries=a.queries, rates=a.rates, pendant_grid=tables.npend, distal_fractions=tables.nfrac,
                max_pitches=tables.max_pitches, chunks=res["nchunks"], chunk_sites=res["chunk_sites"], levels_up=res["nlevels_up"], levels_down=res["nlevels_down"],
                seconds=dict(read=read, eigen_and_tables=eigen_tables, call=call, pack=ms("ms_pack"), copy_in=ms("ms_upload"), matrices=ms("ms_matrices"), sweeps=ms("ms_sweeps"),
                             edge_tables=ms("ms_tables"), scan=ms("ms_scan"), best_edges=ms("ms_topk"), refine=ms("ms_refine"), copy_out=ms("ms_download"), ratios=ratios,
                             tree_and_jplace=tree_jplace),
                scan_products=products, scan_products_per_second=products / ms("ms_scan") if res["ms_scan"] else None,
                placed=sum(1 for p in placements.values() if p), mean_kept=float(np.mean([len(p) for p in placements.values()])) if placements else 0.0)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
