#!/usr/bin/env python
"""Times Simulation.evaluate and write on a synthetic genome: one JSON line with the split of the call (draws on the host, sort and pack,
copy in, kernel, copy out, Python tuples, write), the replicate-set checks per second, and the plain containedMarkerGenes + genomeCheck
loop's time in the same process on a stated subsample of the same draws, with equal results asserted.
usage: python tools/simulation_bench.py --mb 5 --markers 1500 --sets 20 --replicates 20 [--subsample 4] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_genome(mb, markers, sets, seed):
    """(positions, chain, refined chain, genome size): a genome of mb million bases, `sets` marker sets of about `markers` markers each over
    a universe a third larger (most markers once, some twice or three times, a few without a copy), co-located sets of one to four
    markers; the refined twin of a set drops a tenth of its co-located sets."""
    from checkm_amd.markerSets import MarkerSet
    rng = random.Random(seed)
    genomeSize = mb * 1000000
    universe = ["pfam%05d" % k for k in range(markers + markers // 3)]
    positions = {}
    for m in universe:
        copies = rng.choice([0] + [1] * 16 + [2, 2, 3])
        if copies:
            positions[m] = [[p, p + 900] for p in sorted(rng.randrange(0, genomeSize - 1000) for _ in range(copies))]
    chain, refined = [], []
    for s in range(sets):
        mine = rng.sample(universe, min(len(universe), markers))
        cs, at = [], 0
        while at < len(mine):
            n = rng.choice([1, 1, 1, 2, 3, 4])
            cs.append(set(mine[at:at + n])); at += n
        chain.append(MarkerSet("UID%d" % s, "lineage%02d" % s, 20 + 50 * s, cs))
        refined.append(MarkerSet("UID%d" % s, "lineage%02d" % s, 20 + 50 * s, [c for c in cs if rng.random() > 0.1]))
    return positions, chain, refined, genomeSize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=5)
    ap.add_argument("--markers", type=int, default=1500)
    ap.add_argument("--sets", type=int, default=20)
    ap.add_argument("--replicates", type=int, default=20)
    ap.add_argument("--subsample", type=int, default=4, help="draws the plain loop is timed on, evenly spaced over the grid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from checkm_amd.markerSetBuilder import MarkerSetBuilder
    from checkm_amd.markerSets import BinMarkerSets
    from checkm_amd.simulation import Simulation
    positions, chain, refined, genomeSize = synth_genome(a.mb, a.markers, a.sets, seed=18)
    bins = []
    for sets in (chain, refined):
        b = BinMarkerSets("G", BinMarkerSets.TREE_MARKER_SET)
        for ms in sets:
            b.addMarkerSet(ms)
        bins.append(b)
    builder = MarkerSetBuilder(None)
    sim = Simulation(builder)
    builder.genomeChecks(chain[:1], positions, [[0]], [1000])                      # the context, the library and the device are up
    kept = {}
    inner = builder.genomeChecks

    def keep(markerSets, genePositions, contigStartLists, contigLens):
        kept.update(starts=contigStartLists, lens=contigLens)
        kept["out"] = inner(markerSets, genePositions, contigStartLists, contigLens)
        return kept["out"]
    builder.genomeChecks = keep
    random.seed(18); np.random.seed(18)
    t0 = time.perf_counter()
    results = sim.evaluate("G", bins[0], bins[1], positions, genomeSize, a.replicates, ["Bacteria", "Synthetic"])
    wall = time.perf_counter() - t0
    t, d = sim.last_timing, builder.last_sim_timing
    assert d["device"]
    d_out = tempfile.mkdtemp(prefix="ckm_sim_bench_")
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sim.write(results, os.path.join(d_out, "summary.tsv"), os.path.join(d_out, "replicates.tsv.gz"))
    write = time.perf_counter() - t0
    R, S = len(kept["lens"]), len(chain) + len(refined)
    pick = sorted(set(int(k * (R - 1) / max(1, a.subsample - 1)) for k in range(a.subsample))) if R else []
    t0 = time.perf_counter()
    plain = builder._genome_checks_host(chain + refined, positions, [kept["starts"][r] for r in pick], [kept["lens"][r] for r in pick])
    loop = time.perf_counter() - t0
    assert np.array_equal(plain, kept["out"][pick]), "the plain loop and the device disagree"
    starts = sum(len(s) for s in kept["starts"])
    line = dict(tool="simulation_bench", mb=a.mb, markers=a.markers, marker_sets=S, settings=len(results), replicates_per_setting=a.replicates, draws=R, starts=starts,
                distinct_markers=len(set(m for ms in chain + refined for m in ms.getMarkerGenes())), replicate_set_checks=R * S,
                seconds=dict(evaluate=wall, unmodified=t["unmodified"], draws=t["draws"], sort_and_pack=d["pack"], copy_in=d["copy_in"], kernel=d["kernel"], copy_out=d["copy_out"],
                             genome_checks=t["checks"], python_tuples=t["tuples"], write=write),
                rounds=d["rounds"], checks_per_second=dict(kernel=R * S / d["kernel"] if d["kernel"] else None, genome_checks=R * S / t["checks"], evaluate=R * S / wall),
                plain_loop=dict(what="containedMarkerGenes + both genomeCheck modes in Python, same process, one core", draws=pick, replicate_set_checks=len(pick) * S, seconds=loop,
                                checks_per_second=len(pick) * S / loop if loop else None, equal=True))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
