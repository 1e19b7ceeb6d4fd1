#!/usr/bin/env python
"""Times ReducedTree at a given size: a synthetic dereplicated alignment of --rows rows of --columns columns (tests/reducedtree_synth:
clades of 50 rows that differ in about half of their columns, rows of two clades in about 20 of 21, and a planted group of four every
ten rows at 0, limit - 1, limit and limit + 1 differences) with a random tree over its ids, through the steps of ReducedTree.run.
Prints ONE JSON line: the split (ms) read / limits_pack / copy_in / kernel / copy_out / greedy / prune / write, the device call of
every one of --runs runs, row pairs per second and NOMINAL byte comparisons per second (pairs x columns over the kernel's time: the
kernel leaves a tile once every pair of it has reached its limit, so it executes fewer), and the reference's plain Python loop
(reducedTree.plainNearlyIdentical) over all pairs of a subsample of the same rows on this host.
usage: python tools/reducedtree_bench.py --rows 5656 --columns 6988 [--runs 3] [--subsample 60] [--out FILE]
The line is also written to --out (default: profiles/r27_reducedtree_bench_line.json)."""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from checkm_amd import _lib, runtime                                  # noqa: E402
from checkm_amd.genomeTree import readFasta                           # noqa: E402
from checkm_amd.reducedTree import ReducedTree, limitOf, plainNearlyIdentical, prune      # noqa: E402
from checkm_amd.treeParser import Tree, write_newick                  # noqa: E402
from tests import reducedtree_synth as synth                          # noqa: E402


def random_tree_text(rnd, ids):
    nodes = ["%s:%r" % (k, round(rnd.random() * 0.3, 4)) for k in ids]
    while len(nodes) > 1:
        a = nodes.pop(rnd.randrange(len(nodes)))
        b = nodes.pop(rnd.randrange(len(nodes)))
        nodes.append("(%s,%s)%.3f:%r" % (a, b, rnd.random(), round(rnd.random() * 0.3, 4)))
    return nodes[0].rsplit(":", 1)[0] + ";\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5656)
    ap.add_argument("--columns", type=int, default=6988)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--subsample", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_reducedtree_bench_line.json"))
    a = ap.parse_args()
    rnd = random.Random(27)
    d = tempfile.mkdtemp(prefix="ckm_reducedtree_bench_")
    src, out = os.path.join(d, "full"), os.path.join(d, "reduced")
    os.makedirs(src)
    os.makedirs(out)
    text = synth.alignment(27, a.rows, a.columns)
    ids = synth.ids_of(a.rows)
    with open(os.path.join(src, "genome_tree.concatenated.derep.fasta"), "w") as f:
        for k, i in enumerate(ids):
            f.write(">%s\n%s\n" % (i, bytes(text[k]).decode("latin-1")))
    with open(os.path.join(src, "genome_tree.final.tre"), "w") as f:
        f.write(random_tree_text(rnd, ids))
    ctx = runtime.get_ctx()

    t0 = time.perf_counter()
    seqs = readFasta(os.path.join(src, "genome_tree.concatenated.derep.fasta"))
    t1 = time.perf_counter()
    rows = list(seqs.values())
    tables = _lib.NearidTables([s.encode("latin-1") for s in rows], [limitOf(s) for s in rows])
    t2 = time.perf_counter()
    _lib.nearid_run(ctx, _lib.NearidTables(text[:2], [1, 1]))          # (the first call of a process loads the code object)
    calls = [_lib.nearid_run(ctx, tables) for _ in range(max(1, a.runs))]
    o = min(calls, key=lambda c: c["ms_kernel"])
    cached = ReducedTree(runner=lambda t, budget_bytes=0: o)
    t3 = time.perf_counter()
    clusters = cached.nearlyIdentical(seqs)
    t4 = time.perf_counter()
    tree = Tree.from_path(os.path.join(src, "genome_tree.final.tre"))
    keep = [members[0] for members in clusters]
    t5 = time.perf_counter()
    pruned = prune(tree, keep)
    t6 = time.perf_counter()
    with open(os.path.join(out, "genome_tree.tre"), "w") as f:
        f.write(write_newick(pruned) + "\n")
    with open(os.path.join(out, "genome_tree.small.no_internal_labels.tre"), "w") as f:
        f.write(write_newick(pruned, labels=False) + "\n")
    with open(os.path.join(out, "genome_tree.fasta"), "w") as f:
        for k in keep:
            f.write(">%s\n%s\n" % (k, seqs[k]))
    t7 = time.perf_counter()
    random.seed(27)
    whole = ReducedTree()
    with contextlib.redirect_stdout(io.StringIO()):                    # (the run's progress messages: this tool prints one line)
        whole.run(src, os.path.join(d, "whole"))
    t8 = time.perf_counter()

    n = max(2, min(a.subsample, a.rows))
    sub = rows[:n]
    t9 = time.perf_counter()
    near = sum(1 for i in range(n) for j in range(i + 1, n) if plainNearlyIdentical(sub[i], sub[j]))
    t10 = time.perf_counter()

    pairs = a.rows * (a.rows - 1) // 2
    kernel_s = o["ms_kernel"] / 1e3
    line = {"what": "ReducedTree on a synthetic alignment", "rows": a.rows, "columns": a.columns, "row_stride": tables.row_stride, "limit": int(tables.limit[0]),
            "clusters": len(clusters), "largest_cluster": max(len(c) for c in clusters), "bands": o["nbands"], "launches": o["launches"], "blocks": o["blocks"],
            "python_fallbacks": whole.lastInfo["python_fallbacks"], "runs": len(calls),
            "ms": {"read": (t1 - t0) * 1e3, "limits_pack": (t2 - t1) * 1e3, "copy_in": o["ms_upload"], "kernel": o["ms_kernel"], "copy_out": o["ms_download"],
                   "device_call": o["ms_total"], "greedy": (t4 - t3) * 1e3 - (t2 - t1) * 1e3, "prune": (t6 - t5) * 1e3, "write": (t7 - t6) * 1e3, "run_whole": (t8 - t7) * 1e3},
            "kernel_ms_of_every_run": [c["ms_kernel"] for c in calls], "device_call_ms_of_every_run": [c["ms_total"] for c in calls],
            "row_pairs": pairs, "row_pairs_per_s": pairs / kernel_s if kernel_s else None,
            "nominal_byte_comparisons_per_s": pairs * a.columns / kernel_s if kernel_s else None,
            "plain_python": {"rows": n, "row_pairs": n * (n - 1) // 2, "near": near, "s": t10 - t9, "row_pairs_per_s": n * (n - 1) / 2 / (t10 - t9)}}
    out_text = json.dumps(line, sort_keys=True)
    with open(a.out, "w") as f:
        f.write(out_text + "\n")
    print(out_text)


if __name__ == "__main__":
    main()
