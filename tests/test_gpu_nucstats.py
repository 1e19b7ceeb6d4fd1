"""Bin statistics and tetranucleotide signatures on the device: BinStatistics.calculate and GenomicSignatures.calculate against the
reference's output (tests/golden/nucstats_cases.json), against a numpy restatement on synthetic bins beyond the golden sizes (contigs
above 1 Mb, runs of 'N'), run-to-run identity and the reuse of the tree step's result by the analyze step."""
import logging
import re

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd import binStatistics as bs
from checkm_amd import genomicSignatures as gs
from tests.test_nucstats_host import BINS, TETRA, write_case

pytestmark = pytest.mark.gpu


def test_calculate_matches_every_golden_case(tmp_path, caplog):
    """All golden bins in one calculate() call (one output directory), then every recorded tetra file."""
    paths = {name: write_case(tmp_path, case)[0] for name, case in sorted(BINS.items())}
    want = "".join(case["line"] for _name, case in sorted(BINS.items()) if case["line"] is not None)
    with caplog.at_level(logging.ERROR, logger="timestamp"):
        bs.BinStatistics(4).calculate([paths[n] for n in sorted(paths)], str(tmp_path / "out"), "bin_stats.analyze.tsv")
    assert open(str(tmp_path / "out" / "storage" / "bin_stats.analyze.tsv")).read() == want
    assert "no_contig_base" in caplog.text
    for name, text in sorted(TETRA.items()):
        t = str(tmp_path / (name + ".tetra.tsv"))
        gs.GenomicSignatures(4, 2).calculate(paths[name], t)
        assert open(t).read() == text, name


def restated(seqs):
    """(counts [n, 8], pieces per sequence, tetra [n, 136]) by plain numpy / regular expressions."""
    g = gs.GenomicSignatures(4, 1)
    code = np.full(256, -1, dtype=np.int64)
    for ch, v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        code[ch] = v
    canon = np.zeros(256, dtype=np.int64)
    for c in range(256):
        canon[c] = g.kmerToCanonicalIndex["".join("ACGT"[(c >> s) & 3] for s in (6, 4, 2, 0))]
    counts, pieces, tetra = [], [], []
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8)
        up = a & 0xDF
        counts.append([int((up == 65).sum()), int((up == 67).sum()), int((up == 71).sum()), int(((up == 84) | (up == 85)).sum()),
                       int((a == 78).sum()), int((a == 110).sum()), len(s), len(s) - int((a == 78).sum())])
        pieces.append([n for n in (len(p) - p.count(b"N") for p in re.split(b"N{10,}", s)) if n > 0])
        t = np.zeros(136, dtype=np.int64)
        if len(s) >= 4:
            c = code[a]
            w = (c[:-3] << 6) | (c[1:-2] << 4) | (c[2:-1] << 2) | c[3:]
            ok = (c[:-3] >= 0) & (c[1:-2] >= 0) & (c[2:-1] >= 0) & (c[3:] >= 0)
            t = np.bincount(canon[w[ok]], minlength=136)
        tetra.append(t)
    return np.array(counts, dtype=np.uint64), pieces, np.array(tetra, dtype=np.uint32)


def write_fasta(path, contigs, desc=b""):
    with open(path, "wb") as f:
        for cid, s in contigs:
            f.write(b">" + cid.encode() + desc + b"\n" + b"\n".join(s[i:i + 80] for i in range(0, len(s), 80)) + b"\n")
    return str(path)


def synthetic_bins(n_bins, seed):
    rng = np.random.default_rng(seed)
    bins = []
    for b in range(n_bins):
        contigs = []
        for c in range(int(rng.integers(1, 4))):
            n = int(rng.integers(1_000_000, 1_300_000)) if (b % 16 == 0 and c == 0) else int(rng.integers(50, 60_000))
            s = bytearray(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n, p=[.23, .23, .23, .23, .02, .02, .02, .01, .01]).tobytes())
            for _ in range(int(rng.integers(0, 8))):
                at = int(rng.integers(0, len(s) + 1))
                s[at:at] = b"N" * int(rng.integers(8, 30))
            contigs.append(("b%d_c%d" % (b, c), bytes(s)))
        bins.append(contigs)
    return bins


def test_device_pass_matches_a_numpy_restatement(tmp_path):
    bins = synthetic_bins(64, 11)
    paths = [write_fasta(tmp_path / ("bin%02d.fna" % k), contigs) for k, contigs in enumerate(bins)]
    seqs = _lib.NucSeqs(paths)
    flat = [s for contigs in bins for _cid, s in contigs]
    assert seqs.nseq == len(flat) and max(len(s) for s in flat) > 1_000_000
    ctx = runtime.get_ctx()
    r = _lib.nucstats(ctx, seqs, tetra=True)
    r2 = _lib.nucstats(ctx, seqs, tetra=True, tile_bytes=65536)
    seqs.close()
    counts, pieces, tetra = restated(flat)
    assert np.array_equal(r["count"], counts)
    assert np.array_equal(r["tetra"], tetra)
    for i, p in enumerate(pieces):
        assert list(r["piece_len"][int(r["piece_off"][i]):int(r["piece_off"][i + 1])]) == p, i
    for k in ("count", "piece_off", "piece_len", "tetra"):
        assert np.array_equal(r[k], r2[k]), k


def test_tetra_file_matches_a_numpy_restatement_and_repeats_bit_for_bit(tmp_path):
    contigs = [c for b in synthetic_bins(6, 23) for c in b] + [("tiny", b"ACG"), ("allN", b"N" * 40), ("rna", b"ACGUACGU")]
    p = write_fasta(tmp_path / "assembly.fna", contigs, b" description")
    g = gs.GenomicSignatures(4, 8)
    g.calculate(p, str(tmp_path / "a.tsv"))
    g.calculate(p, str(tmp_path / "b.tsv"))
    text = open(str(tmp_path / "a.tsv")).read()
    assert text == open(str(tmp_path / "b.tsv")).read()
    _, _, tetra = restated([s for _c, s in contigs])
    want = "Sequence Id\t" + "\t".join(g.canonicalKmerOrder()) + "\n" + gs.format_rows([c for c, _s in contigs], tetra)
    assert text == want
    assert text.splitlines()[-3].split("\t")[1] == "nan" and text.splitlines()[-2].split("\t")[1] == "nan"


def test_analyze_step_reuses_the_tree_step(tmp_path):
    bins = synthetic_bins(8, 31)
    out = tmp_path / "out"
    (out / "storage").mkdir(parents=True)
    paths = [write_fasta(tmp_path / ("r%d.fna" % k), contigs) for k, contigs in enumerate(bins)]
    b = bs.BinStatistics(1)
    b.calculate(paths, str(out), "bin_stats.tree.tsv")
    assert b.last_timing["reused"] == 0
    b2 = bs.BinStatistics(1)
    b2.calculate(paths, str(out), "bin_stats.analyze.tsv")
    assert b2.last_timing["reused"] == len(paths)
    tree = open(str(out / "storage" / "bin_stats.tree.tsv")).read()
    assert tree == open(str(out / "storage" / "bin_stats.analyze.tsv")).read() and tree.count("\n") == len(paths)
    with open(paths[0], "ab") as f:                  # a changed file is computed again
        f.write(b">extra\nACGTACGT\n")
    b2.calculate(paths, str(out), "bin_stats.analyze.tsv")
    assert b2.last_timing["reused"] == len(paths) - 1


def seam_sequences():
    """Sequences whose runs of 'N' begin at chosen distances in front of every boundary of the device pass: a lane's 16 bytes, a wave
    step's 1024, the tiles' 4096 and 65536, and the end of the sequence.  Every other byte is one of ACGTacgt, up to the last one."""
    rng = np.random.default_rng(2024)

    def filler(n):
        return bytearray(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=n, p=[.22, .22, .22, .22, .03, .03, .03, .03]).tobytes())
    out = []
    # one sequence per seam, run length and distance in front of it: the run's first byte sits at S - d
    for S in (16, 48, 1008, 1024, 2048, 3072, 4096, 8192, 65536, 131072):
        for L in (9, 10, 11, 25):
            for d in range(13):
                s = filler(S + 61 + (L + d) % 7)
                s[S - d:S - d + L] = b"N" * L
                out.append(bytes(s))
    # the end of the sequence: runs that end exactly at, one before and nine before the last byte -- behind a lane, a wave-step and a tile seam
    for n in (200, 1024 + 5, 4096 + 16, 4096 + 3, 65536 + 12):
        for L in (9, 10, 11, 25):
            for back in (0, 1, 9):
                s = filler(n)
                s[n - back - L:n - back] = b"N" * L
                out.append(bytes(s))
    # a sequence that ends INSIDE what would be a longer run at each seam (the bytes behind its end belong to the next sequence or the slack)
    for S in (1024, 4096, 65536):
        for k in (1, 5, 9, 10, 11):
            s = filler(S)
            s[S - k:] = b"N" * k
            out.append(bytes(s))
            s = filler(S + k)
            s[S - 3:] = b"N" * (k + 3)
            out.append(bytes(s))
    out.append(b"N" * 10)                                     # nothing but a run
    out.append(b"N" * 9)                                      # nothing but N, and no run
    out.append(b"N" * 10 + bytes(filler(50)))                 # a run at offset 0
    for S in (64, 1024, 4096):                                # the byte in front of the run is a lower-case n (not part of it), at a seam and one behind it
        for at in (S, S + 1):
            s = filler(S + 80)
            s[at - 1:at] = b"n"
            s[at:at + 10] = b"N" * 10
            out.append(bytes(s))
    s = filler(4096 * 3)                                      # runs that span a whole tile and two seams (4096) / many wave steps
    s[4090:8200] = b"N" * (8200 - 4090)
    out.append(bytes(s))
    return out


def test_runs_of_n_on_every_seam(tmp_path):
    """The halo assembly of the device pass (kernels_nucstats.hip: load_lane -- lane 63's extra load, lane 0's byte in front, the cut at a
    sequence's end) decides whether a run of ten 'N' BEGINS in a lane.  Runs of 9, 10, 11 and 25 begin 0 .. 12 bytes in front of every
    kind of seam, and end at / one before / nine before a sequence's end; three tile sizes (the wave step, the default, 64 KiB) against the
    numpy / regular-expression restatement and against each other."""
    flat = seam_sequences()
    p = write_fasta(tmp_path / "seams.fna", [("s%05d" % k, s) for k, s in enumerate(flat)])
    seqs = _lib.NucSeqs([p])
    assert seqs.nseq == len(flat) and all(seqs.seq(i) == flat[i] for i in range(0, len(flat), 37))
    ctx = runtime.get_ctx()
    counts, pieces, tetra = restated(flat)
    assert sum(len(x) for x in pieces) > len(flat) * 3 // 2           # most sequences are cut in two
    res = {}
    for tile in (0, 1024, 65536):
        r = res[tile] = _lib.nucstats(ctx, seqs, tetra=True, tile_bytes=tile)
        assert np.array_equal(r["count"], counts), tile
        assert np.array_equal(r["tetra"], tetra), (tile, np.nonzero((r["tetra"] != tetra).any(axis=1))[0][:5])
        for i, want in enumerate(pieces):
            assert list(r["piece_len"][int(r["piece_off"][i]):int(r["piece_off"][i + 1])]) == want, (tile, i, len(flat[i]))
    assert res[0]["tiles"] > res[65536]["tiles"] and res[1024]["tiles"] > res[0]["tiles"]
    for tile in (1024, 65536):
        for k in ("count", "piece_off", "piece_len", "tetra"):
            assert np.array_equal(res[0][k], res[tile][k]), (tile, k)
    # a tile size the pass cannot take is refused with an error, not run
    for bad in (24, (1 << 20) + 16):
        with pytest.raises(_lib.CkmError):
            _lib.nucstats(ctx, seqs, tetra=True, tile_bytes=bad)
    seqs.close()
