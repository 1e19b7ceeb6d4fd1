#!/usr/bin/env python
"""Timing of the device bin statistics and tetranucleotide signatures (checkm_amd/binStatistics.py, checkm_amd/genomicSignatures.py).
Prints one JSON line:
  bin_stats  BinStatistics.calculate over --bins synthetic 4 Mb bins (synthdata/synth_genome.py, 40 contigs with runs of 'N'), genes
             called by the library first (genes.gff / genes.faa in bins/<binId>/); the first call is timed (the second one of lineage_wf
             reuses it and is reported too)
  tetra      GenomicSignatures.calculate over one FASTA of --tetra-mb megabases (the bins' contigs repeated under new ids)
Each wall time is split into read, upload, kernel, gff (bin_stats only), host arithmetic and write; kernel_gbs = bytes / kernel time.
--reference <checkm source>: time the reference classes instead, on this host's CPU, over the same bins (no device needed).
usage: python tools/nucstats_bench.py [--bins 64] [--tetra-mb 2048] [--reference DIR]"""
import argparse
import json
import os
import platform
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0        # MI355X peak HBM3E bandwidth (8 TB/s)


def make_bins(work, n):
    from synthdata import synth_genome
    paths = []
    for k in range(n):
        contigs = synth_genome.make_genome(1000 + k, n_contigs=40, contig_len=(90000, 110000), n_runs=3)
        p = os.path.join(work, "bin%04d.fna" % k)
        synth_genome.write_fasta(p, contigs)
        paths.append(p)
    return paths


def call_genes(paths, out):
    from checkm_amd import geneFinder
    jobs = []
    for p in paths:
        d = os.path.join(out, "bins", os.path.splitext(os.path.basename(p))[0])
        os.makedirs(d, exist_ok=True)
        jobs.append((p, d))
    geneFinder.call_bin_files(jobs)


def write_assembly(paths, target_mb, path):
    done, k = 0, 0
    with open(path, "wb") as f:
        while done < target_mb << 20:
            data = open(paths[k % len(paths)], "rb").read().replace(b">", b">r%d_" % k)
            f.write(data)
            done += len(data)
            k += 1
    return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--tetra-mb", type=int, default=2048)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="ckm_nucstats_bench_")
    out = os.path.join(work, "out")
    os.makedirs(os.path.join(out, "storage"), exist_ok=True)
    t0 = time.perf_counter()
    paths = make_bins(work, a.bins)
    res = dict(bins=a.bins, bin_mb=round(sum(os.path.getsize(p) for p in paths) / a.bins / 1e6, 3), setup_s=None)
    if a.reference:
        import multiprocessing
        sys.path.insert(0, a.reference)
        data = tempfile.mkdtemp(prefix="ckm_data_")
        os.makedirs(os.path.join(data, "pfam"))
        open(os.path.join(data, "pfam", "Pfam-A.hmm.dat"), "w").close()
        os.environ["CHECKM_DATA_PATH"] = data
        from checkm.binStatistics import BinStatistics
        from checkm.genomicSignatures import GenomicSignatures
        res.update(mode="reference_cpu", cpu=platform.processor() or platform.machine(), cores=multiprocessing.cpu_count())
        ts = time.perf_counter()
        BinStatistics(multiprocessing.cpu_count()).calculate(paths, out, "bin_stats.tsv")
        res["bin_stats_s"] = round(time.perf_counter() - ts, 3)
        asm = os.path.join(work, "assembly.fna")
        nbytes = write_assembly(paths, a.tetra_mb, asm)
        ts = time.perf_counter()
        GenomicSignatures(4, multiprocessing.cpu_count()).calculate(asm, os.path.join(work, "tetra.tsv"))
        res.update(tetra_bytes=nbytes, tetra_s=round(time.perf_counter() - ts, 3))
        print(json.dumps(res))
        return
    from checkm_amd import runtime
    from checkm_amd.binStatistics import BinStatistics
    from checkm_amd.genomicSignatures import GenomicSignatures
    runtime.get_ctx()
    call_genes(paths, out)
    res["setup_s"] = round(time.perf_counter() - t0, 3)
    b = BinStatistics(16)
    ts = time.perf_counter()
    b.calculate(paths, out, "bin_stats.tree.tsv")
    wall = time.perf_counter() - ts
    t = b.last_timing
    res["bin_stats"] = dict(wall_s=round(wall, 4), read_s=round(t["read"], 4), upload_s=round(t["upload"], 4), kernel_s=round(t["kernel"], 4),
                            gff_s=round(t["gff"], 4), host_s=round(t["host"], 4), write_s=round(t["write"], 4), bytes=t["bytes"],
                            kernel_gbs=round(t["bytes"] / max(t["kernel"], 1e-9) / 1e9, 1))
    ts = time.perf_counter()
    BinStatistics(16).calculate(paths, out, "bin_stats.analyze.tsv")
    res["bin_stats"]["second_call_s"] = round(time.perf_counter() - ts, 4)
    asm = os.path.join(work, "assembly.fna")
    nbytes = write_assembly(paths, a.tetra_mb, asm)
    g = GenomicSignatures(4, 16)
    ts = time.perf_counter()
    g.calculate(asm, os.path.join(work, "tetra.tsv"))
    wall = time.perf_counter() - ts
    t = g.last_timing
    res["tetra"] = dict(file_bytes=nbytes, wall_s=round(wall, 4), read_s=round(t["read"], 4), upload_s=round(t["upload"], 4), kernel_s=round(t["kernel"], 4),
                        host_s=round(t["host"], 4), write_s=round(t["write"], 4), bytes=t["bytes"], kernel_gbs=round(t["bytes"] / max(t["kernel"], 1e-9) / 1e9, 1))
    res["hbm_gbs"] = HBM_GBS
    print(json.dumps(res))
    if os.environ.get("CKM_BENCH_OUT"):
        with open(os.environ["CKM_BENCH_OUT"], "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
