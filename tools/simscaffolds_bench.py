#!/usr/bin/env python
"""Times SimulationScaffolds.evaluate and write on a synthetic genome directory: one JSON line with the split of the run (reading the
directory into IMG's caches, draws on the host, index and pack, copy in, kernel, copy out, Python tuples, write), the (replicate, marker
set) checks per second, and the plain markerGenesOnScaffolds + genomeCheck loop's time in the same process on a stated subsample of the
same draws, with equal results asserted.
usage: python tools/simscaffolds_bench.py --genomes 200 --scaffolds 300 --markers 1500 --sets 20 --replicates 20 [--mode random] [--subsample 4] [--out FILE]"""
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


def synth_case(genomes, scaffolds, markers, sets, seed):
    """(genome -> marker -> [scaffold id per copy], genome -> scaffold id -> length in FASTA order, chain): `genomes` draft genomes of about
    `scaffolds` scaffolds with lengths over two orders of magnitude; a universe a third larger than `markers`, most markers once per
    genome, some twice or three times, a few without a copy; `sets` marker sets of about `markers` markers in co-located sets of one to
    four."""
    from checkm_amd.markerSets import MarkerSet
    rng = random.Random(seed)
    universe = ["pfam%05d" % k for k in range(markers + markers // 3)]
    scaffolds_of, seq_lens = {}, {}
    for g in range(genomes):
        gid = "G%04d" % g
        n = max(1, scaffolds + rng.randrange(-scaffolds // 4, scaffolds // 4 + 1))
        ids = ["%s_s%04d" % (gid, k) for k in range(n)]
        seq_lens[gid] = {s: int(20 * 100 ** rng.random()) for s in ids}
        scaffolds_of[gid] = {}
        for m in universe:
            copies = rng.choice([0] + [1] * 16 + [2, 2, 3])
            if copies:
                scaffolds_of[gid][m] = [ids[rng.randrange(n)] for _ in range(copies)]
    chain = []
    for s in range(sets):
        mine = rng.sample(universe, min(len(universe), markers))
        cs, at = [], 0
        while at < len(mine):
            n = rng.choice([1, 1, 1, 2, 3, 4])
            cs.append(set(mine[at:at + n])); at += n
        chain.append(MarkerSet("UID%d" % s, "lineage%02d" % s, 20 + 50 * s, cs))
    return scaffolds_of, seq_lens, chain


def synth_draws(seq_lens, test, replicates, seed):
    """[(kept scaffolds of `test`, contaminant, its sampled scaffolds)]: seven tenths of the test genome, a tenth of another genome."""
    rng = random.Random(seed)
    others = sorted(set(seq_lens) - set([test]))
    draws = []
    for _ in range(replicates):
        cont = rng.choice(others)
        draws.append(([s for s in seq_lens[test] if rng.random() < 0.7], cont, [s for s in seq_lens[cont] if rng.random() < 0.1]))
    return draws


def write_genome_dir(d, scaffolds_of, seq_lens):
    """The four files of every genome as checkm_amd.img.IMG reads them: one gene per copy, Pfam rows only."""
    for gid, lens in seq_lens.items():
        os.makedirs(os.path.join(d, gid))
        genes = {}
        for m, copies in scaffolds_of[gid].items():
            for s in copies:
                genes.setdefault(s, []).append(m)
        with open(os.path.join(d, gid, gid + ".fna"), "w") as fna, open(os.path.join(d, gid, gid + ".gff"), "w") as gff, \
                open(os.path.join(d, gid, gid + ".pfam.tab.txt"), "w") as pfam, open(os.path.join(d, gid, gid + ".tigrfam.tab.txt"), "w") as tigr:
            pfam.write("gene_oid\tgene_length\tpercent_identity\tquery_start\tquery_end\tsubj_start\tsubj_end\tevalue\tpfam_id\tpfam_name\n")
            tigr.write("gene_oid\tgene_length\tpercent_identity\tquery_start\tquery_end\tevalue\ttigrfam_id\ttigrfam_name\n")
            n = 0
            for s, length in lens.items():
                fna.write(">%s\n%s\n" % (s, "A" * length))
                for m in genes.get(s, []):
                    n += 1
                    gff.write("%s\timg\tCDS\t%d\t%d\t.\t+\t0\tID=%s_%d;locus_tag=x\n" % (s, 10 * n, 10 * n + 9, gid, n))
                    pfam.write("%s_%d\t300\t55.0\t1\t100\t1\t100\t1e-20\t%s\tname\n" % (gid, n, m))
    open(os.path.join(d, "tigrfam2pfam.tsv"), "w").close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=200)
    ap.add_argument("--scaffolds", type=int, default=300)
    ap.add_argument("--markers", type=int, default=1500)
    ap.add_argument("--sets", type=int, default=20)
    ap.add_argument("--replicates", type=int, default=20)
    ap.add_argument("--mode", default="random", choices=["random", "inv_length"])
    ap.add_argument("--subsample", type=int, default=4, help="draws the plain loop is timed on, evenly spaced over the grid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from checkm_amd.img import IMG
    from checkm_amd.markerSetBuilder import MarkerSetBuilder
    from checkm_amd.markerSets import BinMarkerSets, MarkerSet
    from checkm_amd.simulationScaffolds import SimulationScaffolds
    scaffolds_of, seq_lens, chain = synth_case(a.genomes, a.scaffolds, a.markers, a.sets, seed=21)
    rng = random.Random(21)
    refined = [MarkerSet(ms.UID, ms.lineageStr, ms.numGenomes, [c for c in ms.markerSet if rng.random() > 0.1]) for ms in chain]
    d = tempfile.mkdtemp(prefix="ckm_simscaf_bench_")
    write_genome_dir(d, scaffolds_of, seq_lens)
    bins = []
    for sets in (chain, refined):
        b = BinMarkerSets("G", BinMarkerSets.TREE_MARKER_SET)
        for ms in sets:
            b.addMarkerSet(ms)
        bins.append(b)
    ids = sorted(seq_lens)
    test = ids[0]
    builder = MarkerSetBuilder(IMG(None, os.path.join(d, "tigrfam2pfam.tsv"), d))
    t0 = time.perf_counter()
    builder.precomputeGenomeSeqLens(ids)
    builder.precomputeGenomeFamilyScaffolds(ids)
    read = time.perf_counter() - t0
    assert {m: sorted(v) for m, v in builder.img.cachedGenomeFamilyScaffolds[test].items()} == {m: sorted(v) for m, v in scaffolds_of[test].items()}
    sim = SimulationScaffolds(builder, mode=a.mode)
    builder.scaffoldChecks(chain[:1], test, [([], None, [])])                      # the context, the library and the device are up
    kept = {}
    inner = builder.scaffoldChecks

    def keep(markerSets, testGenomeId, draws):
        kept["draws"] = draws
        kept["out"] = inner(markerSets, testGenomeId, draws)
        return kept["out"]
    builder.scaffoldChecks = keep
    random.seed(21); np.random.seed(21)
    t0 = time.perf_counter()
    results = sim.evaluate(test, bins[0], bins[1], ids, a.replicates, ["Bacteria", "Synthetic"])
    wall = time.perf_counter() - t0
    t, dv = sim.last_timing, builder.last_scaffold_timing
    assert dv["device"]
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sim.write(results, os.path.join(d, "summary.tsv"), os.path.join(d, "replicates.tsv.gz"))
    write = time.perf_counter() - t0
    R, S = len(kept["draws"]), len(chain) + len(refined)
    pick = sorted(set(int(k * (R - 1) / max(1, a.subsample - 1)) for k in range(a.subsample))) if R else []
    t0 = time.perf_counter()
    plain = builder._scaffold_checks_host(chain + refined, test, [kept["draws"][r] for r in pick])
    loop = time.perf_counter() - t0
    assert np.array_equal(plain, kept["out"][pick]), "the plain loop and the device disagree"
    line = dict(tool="simscaffolds_bench", mode=a.mode, genomes=a.genomes, scaffolds=a.scaffolds, markers=a.markers, marker_sets=S, settings=len(results),
                replicates_per_setting=a.replicates, draws=R, kept_scaffolds=sum(len(x[0]) + len(x[2]) for x in kept["draws"]),
                distinct_markers=len(set(m for ms in chain + refined for m in ms.getMarkerGenes())), replicate_set_checks=R * S,
                seconds=dict(read=read, evaluate=wall, unmodified=t["unmodified"], draws=t["draws"], index_and_pack=dv["pack"], copy_in=dv["copy_in"], kernel=dv["kernel"],
                             copy_out=dv["copy_out"], scaffold_checks=t["checks"], python_tuples=t["tuples"], write=write),
                rounds=dv["rounds"], checks_per_second=dict(kernel=R * S / dv["kernel"] if dv["kernel"] else None, scaffold_checks=R * S / t["checks"], evaluate=R * S / wall),
                plain_loop=dict(what="markerGenesOnScaffolds for both genomes + both genomeCheck modes in Python, same process, one core", draws=pick,
                                replicate_set_checks=len(pick) * S, seconds=loop, checks_per_second=len(pick) * S / loop if loop else None, equal=True))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
