#!/usr/bin/env python
"""Times GeneTrees' two tests at a given size: a synthetic directory of --trees gene trees of --leaves leaves each (random joins with
multifurcations, a quarter of the leaves second copies of a genome), read, packed and scored in one device call per test, then the
reports on the host.  Prints ONE JSON line: the split (ms) read_parse / ranges_pack / copy_in / consistency / flags / conspecific /
copy_out of the bare device call, then each test whole through the class (read, reroot, pack, device call, reports and file writes:
paralog_test_whole / consistency_test_whole), (node, class) quotients per second (the internal nodes of every tree times its classes over the consistency
kernel's time), pairs per second, and the plain Python loop (geneTrees.plainTreeTests) on a subsample of the same trees on this host.
usage: python tools/genetrees_bench.py --trees 200 --leaves 3000 [--subsample 2] [--out FILE]
The line is also written to --out (default: the next free profiles/rNN_genetrees_bench_line.json)."""
import argparse
import glob
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from checkm_amd import _lib, geneTrees, runtime                       # noqa: E402
from checkm_amd.geneTrees import GeneTrees                            # noqa: E402
from tests import genetrees_synth as synth                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--leaves", type=int, default=3000)
    ap.add_argument("--subsample", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ngenomes = max(2, a.leaves * 3 // 4)
    md = synth.metadata(ngenomes, nphyla=30, nclasses=60)
    d = tempfile.mkdtemp(prefix="ckm_genetrees_bench_")
    tree_dir = os.path.join(d, "trees")
    os.makedirs(tree_dir)
    specs = [("PF%05d.tre" % k, "random", a.leaves, ngenomes, (), 0.05) for k in range(a.trees)]
    for name, text in synth.forest(26, specs):
        open(os.path.join(tree_dir, name), "w").write(text + "\n")
    desc = {"PF%05d" % k: ["short", "long"] for k in range(a.trees)}
    ctx = runtime.get_ctx()

    t0 = time.perf_counter()
    texts = [(f, open(os.path.join(tree_dir, f)).read()) for f in sorted(os.listdir(tree_dir))]
    roots = [(f, geneTrees.parse_newick(t)) for f, t in texts]
    t1 = time.perf_counter()
    packed = [geneTrees.packTree(f, r, md, geneTrees.genomeIdOfGene) for f, r in roots]
    tables = geneTrees.forestTables(packed)
    t2 = time.perf_counter()
    _lib.genetree_run(ctx, geneTrees.forestTables(packed[:1]))         # (the first call of a process loads the code object)
    o = _lib.genetree_run(ctx, tables)
    t3 = time.perf_counter()
    quotients = sum(int(p.internal.sum()) * sum(len(c) for c in p.classes) for p in packed)

    gt = GeneTrees()
    t4 = time.perf_counter()
    records = gt.paralogTest(tree_dir, md, 0.01, ".tre", os.path.join(d, "conspecific"))
    t5 = time.perf_counter()
    gt.consistencyTest(tree_dir, md, desc, 0.86, 20, ".tre", os.path.join(d, "consistency.tsv"), os.path.join(d, "final"))
    t6 = time.perf_counter()
    info = gt.lastInfo

    sub = packed[:max(1, min(a.subsample, len(packed)))]
    t7 = time.perf_counter()
    for p in sub:
        geneTrees.plainTreeTests(p)
    t8 = time.perf_counter()
    sub_quotients = sum(int(p.internal.sum()) * sum(len(c) for c in p.classes) for p in sub)

    line = {"what": "GeneTrees on a synthetic forest", "trees": a.trees, "leaves": a.leaves, "nodes": int(tables.node_off[-1]), "classes": tables.nclasses, "pairs": tables.npairs,
            "groups": tables.ngroups, "rounds": o["nrounds"], "launches": o["launches"], "python_trees": info["python_trees"],
            "ms": {"read_parse": (t1 - t0) * 1e3, "ranges_pack": (t2 - t1) * 1e3, "copy_in": o["ms_upload"], "consistency": o["ms_consistency"], "flags": o["ms_flags"],
                   "conspecific": o["ms_conspecific"], "copy_out": o["ms_download"], "device_call": o["ms_total"], "device_call_wall": (t3 - t2) * 1e3,
                   "paralog_test_whole": (t5 - t4) * 1e3, "consistency_test_whole": (t6 - t5) * 1e3},
            "node_class_quotients": quotients, "quotients_per_s": quotients / (o["ms_consistency"] / 1e3) if o["ms_consistency"] else None,
            "pairs_per_s": tables.npairs / (o["ms_flags"] / 1e3) if o["ms_flags"] else None,
            "retained_by_paralog_test": sum(r["retained"] for r in records),
            "plain_python": {"trees": len(sub), "s": t8 - t7, "quotients_per_s": sub_quotients / (t8 - t7)}}
    text = json.dumps(line, sort_keys=True)
    out = a.out
    if out is None:
        used = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_genetrees_bench_line.json"))) if m]
        out = os.path.join(ROOT, "profiles", "r%02d_genetrees_bench_line.json" % (max(used) + 1 if used else 26))
    with open(out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
