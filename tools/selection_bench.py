#!/usr/bin/env python
"""Times MarkerSetSelection.selectMarkerSet on a synthetic node: one JSON line with the split of the call (chains, positions, pack, copy in,
kernel, copy out, numpy, write), the draws per second, and the same node with draws='host' (random.uniform, sampleGenome and genomeChecks)
on a stated subsample of its test genomes and replicates.  The chain, the gene positions and the genome sizes are made in memory: the
marker passes of the chain and the reading of IMG files are not part of this measurement, and the line says so.
usage: python tools/selection_bench.py --genomes 100 --mb 5 --markers 1500 --sets 6 [--replicates 100] [--host-genomes 2 --host-replicates 10] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_node(genomes, mb, markers, sets, seed):
    """(marker sets of the chain, gene positions per test genome, genome sizes): `sets` marker sets of about `markers` markers each over a
    universe a third larger, co-located sets of one to four markers; per genome most markers once, some twice or three times, a few without
    a copy, anywhere in about mb million bases."""
    from checkm_amd.markerSets import MarkerSet
    rng = random.Random(seed)
    universe = ["pfam%05d" % k for k in range(markers + markers // 3)]
    chain = []
    for s in range(sets):
        mine = rng.sample(universe, min(len(universe), markers))
        cs, at = [], 0
        while at < len(mine):
            n = rng.choice([1, 1, 1, 2, 3, 4])
            cs.append(set(mine[at:at + n])); at += n
        chain.append(MarkerSet("UID%d" % s, "UID%d | lineage%02d" % (s, s), 20 + 50 * s, cs))
    positions, sizes = [], []
    for _ in range(genomes):
        size = mb * 1000000 + rng.randrange(0, 500000)
        mine = {}
        for m in universe:
            copies = rng.choice([0] + [1] * 16 + [2, 2, 3])
            if copies:
                mine[m] = [[p, p + 900] for p in sorted(rng.randrange(0, size - 1000) for _ in range(copies))]
        positions.append(mine); sizes.append(size)
    return chain, positions, sizes


class _Img(object):
    """geneDistTable from memory."""
    def __init__(self, positions):
        self.positions = positions

    def geneDistTable(self, genomeIds, markerGenes, spacingBetweenContigs=0):
        return {g: {m: p for m, p in self.positions[g].items() if m in markerGenes} for g in genomeIds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100)
    ap.add_argument("--mb", type=int, default=5)
    ap.add_argument("--markers", type=int, default=1500)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--host-genomes", type=int, default=2)
    ap.add_argument("--host-replicates", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from checkm_amd.markerSetBuilder import MarkerSetBuilder
    from checkm_amd.markerSetSelection import MarkerSetSelection
    from checkm_amd.markerSets import BinMarkerSets
    from checkm_amd.treeParser import read_newick
    G = max(a.genomes, 5)
    sets, positions, sizes = synth_node(G, a.mb, a.markers, a.sets, seed=22)
    ids = ["G%03d" % g for g in range(G)]
    chain = BinMarkerSets("UID3|p__P|70", BinMarkerSets.TREE_MARKER_SET)
    for ms in sets:
        chain.addMarkerSet(ms)
    tree = read_newick("((%s)UID5|c__A|90,(%s)UID6||80)UID3|p__P|70;" % (",".join("IMG_" + g for g in ids), ",".join("IMG_other%d" % k for k in range(G + 1))))
    builder = MarkerSetBuilder(_Img(dict(zip(ids, positions))))
    sel = MarkerSetSelection(builder)
    sel._genome_size = lambda g: sizes[ids.index(g)]
    builder.sampledGenomeChecks(sets[:1], positions[:1], sizes[:1], 1, 10000)                    # the context, the library and the device are up
    assert builder.last_select_timing["device"]
    random.seed(22); np.random.seed(22)
    t0 = time.perf_counter()
    result = sel.selectMarkerSet(tree, tree.root, 0.97, 0.97, draws="device", seed=22, maxTestGenomes=G, repsPerGenome=a.replicates, chain=chain)
    wall = time.perf_counter() - t0
    t = dict(sel.last_timing)
    assert builder.last_select_timing["device"]
    path = os.path.join(tempfile.mkdtemp(prefix="ckm_selection_bench_"), "simInferBestMarkerSet.tsv")
    t0 = time.perf_counter()
    with open(path, "w") as f:
        f.write(sel.HEADER)
        f.write(result[0] + "\t%s\t%.2f\t%.2f\t%.2f\t%.2f\n" % result[1:])
    t["write"] = time.perf_counter() - t0
    draws = G * a.replicates
    hg, hr = min(a.host_genomes, G), a.host_replicates
    random.seed(22); np.random.seed(22)
    t0 = time.perf_counter()
    host = sel.selectMarkerSet(tree, tree.root, 0.97, 0.97, draws="host", maxTestGenomes=hg, repsPerGenome=hr, chain=chain)
    host_wall = time.perf_counter() - t0
    th = sel.last_timing
    line = dict(tool="selection_bench", genomes=G, mb=a.mb, markers=a.markers, marker_sets=len(sets), replicates_per_genome=a.replicates, draws=draws,
                contigs_per_genome=sizes[0] // sel.simContigLen, distinct_markers=len(chain.getMarkerGenes()), draw_set_checks=draws * len(sets),
                not_measured="the marker passes of the chain (it is given) and the reading of IMG files (positions and sizes come from memory)",
                seconds=dict(select_marker_set=wall, chains=t["chains"], positions=t["positions"], pack=t["pack"], copy_in=t["copy_in"], kernel=t["kernel"], copy_out=t["copy_out"],
                             numpy=t["numpy"], write=t["write"]),
                rounds=builder.last_select_timing["rounds"], draws_per_second=dict(kernel=draws / t["kernel"] if t["kernel"] else None, select_marker_set=draws / wall),
                best=dict(uid=result[1], mean_delta_comp=float(result[2]), mean_delta_cont=float(result[4])),
                host_draws=dict(what="the same node with draws='host': random.uniform and sampleGenome per replicate, genomeChecks per genome on the device", genomes=hg,
                                replicates_per_genome=hr, draws=hg * hr, seconds=dict(select_marker_set=host_wall, draws=th["draws"], genome_checks=th["checks"], positions=th["positions"]),
                                draws_per_second=hg * hr / host_wall, best_uid=host[1]))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
