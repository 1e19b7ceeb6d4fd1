#!/usr/bin/env python
"""Times GenomeTree at a given size: a synthetic alignment (every row a mutated copy of an earlier one, a tenth of the cells gaps), the
tree of the alignment and of every bootstrap replicate in one device call, then the supports and the Newick text on the host.  Prints ONE
JSON line: the split (ms) read / copy_in / gather / counts / distances / joins / copy_out / supports / newick, column comparisons per
second (trees x row pairs x columns over the counts' time), matrix cells scanned per second (the active upper triangle of every join
round over the joins' time), the launches, and a plain numpy neighbour joining of a subsample of the same distance matrix on this host.
usage: python tools/genometree_bench.py --leaves 5656 --columns 6988 --bootstraps 100 [--subsample 512] [--out FILE]
The line is also written to --out (default: the next free profiles/rNN_genometree_bench_line.json)."""
import argparse
import glob
import json
import os
import random
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from checkm_amd import _lib, runtime                                  # noqa: E402
from checkm_amd.genomeTree import GenomeTree, _newick                        # noqa: E402

AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def synthetic(leaves, columns, seed):
    rng = np.random.RandomState(seed)
    state = np.zeros((leaves, columns), dtype=np.uint8)
    state[0] = rng.randint(0, 20, columns)
    for k in range(1, leaves):
        src = state[rng.randint(0, k)]
        hit = rng.random_sample(columns) < 0.08
        state[k] = np.where(hit, (src + rng.randint(1, 20, columns)) % 20, src)
    text = AA[state]
    text[rng.random_sample((leaves, columns)) < 0.10] = ord("-")
    return {"g%05d" % k: text[k].tobytes() for k in range(leaves)}


def numpy_nj(D):
    """Saitou-Nei / Studier-Keppler on a copy of D, R kept up to date; returns the joins (seconds are the caller's)."""
    D = np.array(D)
    n = D.shape[0]
    act = np.arange(n)
    R = D.sum(axis=1)
    joins = []
    while len(act) > 3:
        m = len(act)
        sub = D[np.ix_(act, act)]
        Q = (m - 2) * sub - R[act][:, None] - R[act][None, :]
        Q[np.tril_indices(m)] = np.inf
        a, b = np.unravel_index(np.argmin(Q), Q.shape)
        i, j = act[a], act[b]
        new = (D[i] + D[j] - D[i, j]) / 2
        R -= D[i] + D[j]
        R += new
        D[i, :], D[:, i] = new, new
        D[i, i] = 0.0
        act = np.delete(act, b)
        R[i] = D[i, act].sum()
        joins.append((int(i), int(j)))
    return joins


def next_profile():
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d_genometree_bench_line.json" % (max(taken + [0]) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=5656)
    ap.add_argument("--columns", type=int, default=6988)
    ap.add_argument("--bootstraps", type=int, default=100)
    ap.add_argument("--subsample", type=int, default=512)
    ap.add_argument("--model", default="kimura")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * a.leaves + 1000))
    seqs = synthetic(a.leaves, a.columns, a.seed)
    gt = GenomeTree()
    t0 = time.perf_counter()
    random.seed(a.seed)
    cols = gt.bootstrapColumns(a.columns, a.bootstraps) if a.bootstraps else None
    ids, tables = gt._tables(seqs, cols=cols, base=True, model=a.model)
    ms_read = (time.perf_counter() - t0) * 1e3
    ctx = runtime.get_ctx()
    _lib.gtree_run(ctx, _lib.GtreeTables(text=b"ACDEACDFACDG", nrows=3, ncols=4))          # the context's first call (module load) is not the pass
    t0 = time.perf_counter()
    r = _lib.gtree_run(ctx, tables, dist=True)
    ms_device = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    splits = [gt._splits_of_merges(len(ids), r["merge_ij"][k]) for k in range(1, 1 + a.bootstraps)]
    root = gt._tree_of(ids, r["merge_ij"][0], r["merge_len"][0])
    ms_tree = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    text = _newick(root)
    ms_newick = (time.perf_counter() - t0) * 1e3 + ms_tree
    t0 = time.perf_counter()
    text = gt.supportTree(text, ids, splits)
    ms_supports = (time.perf_counter() - t0) * 1e3
    sub = min(a.subsample, a.leaves)
    t0 = time.perf_counter()
    numpy_nj(r["dist"][:sub, :sub])
    ms_numpy = (time.perf_counter() - t0) * 1e3
    n, trees = a.leaves, 1 + a.bootstraps
    cells = sum(m * (m - 1) // 2 for m in range(4, n + 1))
    line = dict(leaves=n, columns=a.columns, bootstraps=a.bootstraps, model=a.model, trees=trees, batches=r["nrounds"], launches=r["launches"],
                ms=dict(read=round(ms_read, 3), copy_in=round(r["ms_upload"], 3), gather=round(r["ms_gather"], 3), counts=round(r["ms_counts"], 3),
                        distances=round(r["ms_dist"], 3), joins=round(r["ms_joins"], 3), copy_out=round(r["ms_download"], 3), supports=round(ms_supports, 3),
                        newick=round(ms_newick, 3), device_call=round(ms_device, 3)),
                column_comparisons_per_s=trees * (n * (n - 1) // 2) * a.columns / max(r["ms_counts"], 1e-9) * 1e3,
                matrix_cells_scanned_per_s=trees * cells / max(r["ms_joins"], 1e-9) * 1e3,
                numpy_join=dict(leaves=sub, ms=round(ms_numpy, 3), cells_per_s=sum(m * (m - 1) // 2 for m in range(4, sub + 1)) / max(ms_numpy, 1e-9) * 1e3),
                newick_bytes=len(text), runs=1)
    out = json.dumps(line, sort_keys=True)
    print(out)
    path = a.out or next_profile()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(out + "\n")


if __name__ == "__main__":
    main()
