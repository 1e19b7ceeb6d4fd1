#!/usr/bin/env python
"""Times MarkerSetBuilder's two device passes on a synthetic table: G genomes, C families, Q queries (clades: stretches of the genome
order), the default thresholds of buildMarkerSet (0.97 / 0.97, 5000 bases, 0.95).  Needs an MI355X; prints ONE JSON line.

The table is made here from a seed: six of ten families are core (present in 99.8 % of the genomes), the others accessory (40 %); one
present family in a hundred (--multicopy) has 2 to 5 copies; families lie in groups of four 1500 bases apart, the groups 20 kb apart, each
genome with its own jitter, and two cells in a hundred are rearranged to a random place.  Nothing is read from disk, so "read" is the time to make the
table's arrays.  Per phase: one warm-up call, then --repeats calls on the resident table; median and range (min, max) in seconds.  The
phases are the library's own HIP-event timings (table copy in, marker pass, pack, count, scan, fill, copy out); union_find is
MarkerSetBuilder.colocatedSets over every query, python the rest of a call's wall time.  pair_tests_per_second is the (genome, marker
pair) tests of the co-location pass over the median time of its count kernel alone.
usage: python tools/markerset_bench.py --genomes 2000 --families 4000 --queries 200 [--repeats 5] [--multicopy 0.01]
                                       [--out profiles/r17_markerset_bench_line.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_table(genomes, families, seed, multicopy=0.01):
    """(count_class [G, C] uint8, pos_off [G * C + 1] uint64, pos int64) of the synthetic table."""
    rng = np.random.default_rng(seed)
    core = rng.random(families) < 0.6
    present = rng.random((genomes, families)) < np.where(core, 0.998, 0.4)[None, :]
    multi = present & (rng.random((genomes, families)) < multicopy)
    ncopy = present.astype(np.int64) + multi * rng.integers(1, 5, size=(genomes, families))
    base = np.arange(families, dtype=np.int64) * 1500 + (np.arange(families, dtype=np.int64) // 4) * 20000
    first = base[None, :] + rng.integers(-200, 201, size=(genomes, families)) + 1000
    moved = rng.random((genomes, families)) < 0.02
    first = np.where(moved, rng.integers(0, 1 << 30, size=(genomes, families)), first)
    pos_off = np.zeros(genomes * families + 1, dtype=np.uint64)
    np.cumsum(ncopy.reshape(-1), out=pos_off[1:])
    pos = rng.integers(0, 1 << 30, size=int(pos_off[-1]), dtype=np.int64)
    has = ncopy.reshape(-1) > 0
    pos[pos_off[:-1][has].astype(np.int64)] = first.reshape(-1)[has]
    return np.minimum(ncopy, 2).astype(np.uint8), pos_off, pos


def synth_queries(genomes, queries, seed):
    """Clades: stretches of 5 to a fifth of the genomes."""
    rng = np.random.default_rng(seed + 1)
    out = []
    for _ in range(queries):
        n = int(rng.integers(min(5, genomes), max(min(5, genomes) + 1, genomes // 5 + 1)))
        lo = int(rng.integers(0, genomes - n + 1))
        out.append(list(range(lo, lo + n)))
    return out


def synth_dist_table(genomes, markers, seed):
    """The same table as a geneDistTable of the reference: genome -> family -> [[start, end], ...], every family a marker."""
    cls, pos_off, pos = synth_table(genomes, markers, seed)
    off, p = pos_off.tolist(), pos.tolist()
    return {"G%05d" % g: {"pfam%05d" % f: [[s, s + 900] for s in p[off[g * markers + f]:off[g * markers + f + 1]]]
                          for f in range(markers) if off[g * markers + f + 1] > off[g * markers + f]} for g in range(genomes)}


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=2000)
    ap.add_argument("--families", type=int, default=4000)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--multicopy", type=float, default=0.01, help="share of the present cells with 2 to 5 copies")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from checkm_amd import _lib
    from checkm_amd.markerSetBuilder import MarkerSetBuilder
    if _lib.device_count() < 1:
        raise SystemExit("markerset_bench needs a GPU: no HIP device is visible")
    t0 = time.perf_counter()
    cls, pos_off, pos = synth_table(a.genomes, a.families, a.seed, a.multicopy)
    glists = synth_queries(a.genomes, a.queries, a.seed)
    read = time.perf_counter() - t0
    ctx = _lib.Context(0)
    table = _lib.MsetTable(ctx, cls, pos_off, pos)
    copy_in = [table.ms_upload / 1e3]
    tU, tS = [0.97 * len(g) for g in glists], [0.97 * len(g) for g in glists]
    phases = dict((k, []) for k in ("markers", "pack", "count", "scan", "fill", "copy_out", "union_find", "python", "wall"))
    b = MarkerSetBuilder()
    names = ["pfam%05d" % f for f in range(a.families)]
    for rep in range(a.repeats + 1):
        w0 = time.perf_counter()
        m = _lib.mset_markers(ctx, table, glists, tU, tS)
        mlists = [np.nonzero(row & 1)[0].tolist() for row in m["flag"]]
        r = _lib.mset_colocated(ctx, table, glists, mlists, 5000, 0.95)
        u0 = time.perf_counter()
        off, pi, pj = r["pair_off"].tolist(), r["i"].tolist(), r["j"].tolist()
        nsets = 0
        for q, ml in enumerate(mlists):
            pairs = [names[ml[pi[x]]] + "-" + names[ml[pj[x]]] for x in range(off[q], off[q + 1])]
            nsets += len(b.colocatedSets(pairs, [names[f] for f in ml]))
        uf = time.perf_counter() - u0
        wall = time.perf_counter() - w0
        if rep == 0:
            continue                                   # warm-up: code objects, first allocations
        dev = dict(markers=m["ms_markers"], pack=r["ms_pack"], count=r["ms_count"], scan=r["ms_scan"], fill=r["ms_fill"],
                   copy_out=m["ms_download"] + r["ms_download"])
        for k, v in dev.items():
            phases[k].append(v / 1e3)
        phases["union_find"].append(uf)
        phases["python"].append(wall - uf - (sum(dev.values()) + m["ms_upload"] + r["ms_upload"]) / 1e3)
        phases["wall"].append(wall)
    for _ in range(a.repeats):
        table.close()
        table = _lib.MsetTable(ctx, cls, pos_off, pos)
        copy_in.append(table.ms_upload / 1e3)
    line = dict(what="MarkerSetBuilder device passes, synthetic table", device="MI355X (gfx950)", genomes=a.genomes, families=a.families, queries=a.queries,
                repeats=a.repeats, seed=a.seed, multicopy=a.multicopy, markers_per_query=spread([len(x) for x in mlists]), genomes_per_query=spread([len(x) for x in glists]),
                pair_tests=int(r["tests"]), reported_pairs=int(r["npairs"]), sets=nsets, rounds=int(r["nrounds"]), batches=int(r["nbatches"]),
                seconds=dict(dict((k, spread(v)) for k, v in phases.items()), read=read, table_copy_in=spread(copy_in)),
                pair_tests_per_second=int(r["tests"]) / statistics.median(phases["count"]) if statistics.median(phases["count"]) > 0 else None)
    table.close()
    ctx.close()
    text = json.dumps(line)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
