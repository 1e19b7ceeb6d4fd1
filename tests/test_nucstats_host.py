"""Bin statistics and tetranucleotide signatures without a device: the readFasta-rule reader (ckm_nucseq_read), the gene files of a bin
(ckm_bin_genes_read), the tile logic of the device pass run by the host executor (tests/emu/nucstats_emu.cpp) with tiles forced small so
that the seams fall inside runs of 'N' and 4-mers, and the Python layer -- all against the reference's own output
(tests/golden/nucstats_cases.json, tools/gen_nucstats_golden.py)."""
import gzip
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import binStatistics as bs
from checkm_amd import genomicSignatures as gs
from tests.emu import nucstats as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "nucstats_cases.json")))
BINS = {b["name"]: b for b in GOLD["bins"]}
TETRA = {t["name"]: t["text"] for t in GOLD["tetra"]}


def write_case(tmp, case):
    """The case's bin file and bins/<name>/genes.* under tmp; returns (fasta path, out dir)."""
    out = tmp / "out"
    (out / "storage").mkdir(parents=True, exist_ok=True)
    path = tmp / (case["name"] + (".fna.gz" if case["gz"] else ".fna"))
    data = case["fasta"].encode("utf-8")
    if case["gz"]:
        with gzip.open(str(path), "wb") as f:
            f.write(data)
    else:
        path.write_bytes(data)
    if case["gff"] is not None:
        d = out / "bins" / case["name"]
        d.mkdir(parents=True, exist_ok=True)
        (d / "genes.gff").write_text(case["gff"])
        (d / "genes.faa").write_text(case["faa"])
    return str(path), str(out)


@pytest.mark.parametrize("name", sorted(BINS))
def test_reader_view_is_readfasta(tmp_path, name):
    path, _ = write_case(tmp_path, BINS[name])
    b = _lib.NucSeqs([path])
    got = [[i, b.seq(k).decode("utf-8")] for k, i in enumerate(b.ids())]
    assert got == BINS[name]["view"]
    assert all(int(o) % 16 == 0 for o in b.seq_off)
    b.close()


def test_reader_refuses_invalid_utf8_and_text_before_a_header(tmp_path):
    p = tmp_path / "bad.fna"
    p.write_bytes(b">a\nACGT\xff\n")
    with pytest.raises(_lib.CkmError) as e:
        _lib.NucSeqs([str(p)])
    assert e.value.code == -3 and "UTF-8" in str(e.value)
    p.write_bytes(b"ACGT\n>a\nACGT\n")
    with pytest.raises(_lib.CkmError):
        _lib.NucSeqs([str(p)])
    with pytest.raises(_lib.CkmError) as e:
        _lib.NucSeqs([str(tmp_path / "missing.fna")])
    assert e.value.code == -2


def result_of(case, count, piece_off, piece_len, tmp_path):
    """The bin line BinStatistics.calculate writes, from per-sequence results of one bin (device or host executor)."""
    path, out = write_case(tmp_path, case)
    b = _lib.NucSeqs([path])
    genes = _lib.bin_genes(b, [os.path.join(out, "bins", case["name"], "genes.gff")], [os.path.join(out, "bins", case["name"], "genes.faa")])
    b.close()
    st = bs.BinStatistics(1)._bin_stats(case["name"], dict(count=count, piece_off=piece_off, piece_len=piece_len), 0, len(count), genes[0])
    return None if st is None else case["name"] + "\t" + str(st) + "\n"


@pytest.mark.parametrize("tile", [16, 32, 48, 1024, 65536])
def test_host_executor_tiles_match_the_reference(tmp_path, tile):
    for name, case in sorted(BINS.items()):
        seqs = [v.encode("utf-8") for _k, v in case["view"]]
        r = emu.nucstats(seqs, tile)
        d = tmp_path / ("%s_%d" % (name, tile))
        d.mkdir()
        assert result_of(case, r["count"], r["piece_off"], r["piece_len"], d) == case["line"], (name, tile)
        if name not in TETRA:
            continue
        ids = [k for k, _v in case["view"]]
        header = "Sequence Id\t" + "\t".join(gs.GenomicSignatures(4, 1).canonicalKmerOrder()) + "\n"
        assert header + gs.format_rows(ids, r["tetra"]) == TETRA[name], (name, tile)


def test_host_executor_agrees_across_tile_sizes():
    rng = np.random.default_rng(5)
    seqs = []
    for _ in range(12):
        s = bytearray(rng.choice(list(b"ACGTacgtNnRY"), size=int(rng.integers(1, 5000))).tobytes())
        for _ in range(int(rng.integers(0, 6))):
            at = int(rng.integers(0, len(s) + 1))
            s[at:at] = b"N" * int(rng.integers(5, 40))
        seqs.append(bytes(s))
    ref = emu.nucstats(seqs, 65536)
    for tile in (16, 64, 112, 2048):
        r = emu.nucstats(seqs, tile)
        for k in ("count", "piece_off", "piece_len", "tetra"):
            assert np.array_equal(r[k], ref[k]), (tile, k)


def test_python_methods_on_dicts_follow_the_reference(tmp_path):
    """calculateGC / calculateSeqStats / calculateCodingDensity on readFasta dicts give the golden line's values."""
    for name, case in sorted(BINS.items()):
        if case["line"] is None:
            continue
        want = eval(case["line"].split("\t", 1)[1])
        seqs = dict((k, v) for k, v in case["view"])
        b = bs.BinStatistics(1)
        gc, std = b.calculateGC(seqs)
        assert (gc, std) == (want["GC"], want["GC std"]), name
        st = b.calculateSeqStats(seqs)
        assert st[2] == want["Genome size"] and st[3] == want["N50 (scaffolds)"] and st[4] == want["N50 (contigs)"], name
        assert float(st[5]) == want["Mean scaffold length"] and float(st[6]) == want["Mean contig length"] and st[7] == want["# contigs"], name
        assert st[8] == want["# ambiguous bases"], name
        d = tmp_path / name
        d.mkdir()
        _, out = write_case(d, case)
        cd = b.calculateCodingDensity(os.path.join(out, "bins", name), seqs, st[2])
        assert cd == (want["Coding density"], want["Translation table"], want["# predicted genes"]), name


def test_sequence_stats_without_genes_faa_raises_name_error(tmp_path):
    case = BINS["crlf"]
    path, out = write_case(tmp_path, case)
    b = bs.BinStatistics(1)
    st = b.sequenceStats(out, path)
    assert set(st) == {"c1", "c2"} and st["c1"]["Length"] == 300 and "# ORFs" in st["c1"]
    os.remove(os.path.join(out, "bins", "crlf", "genes.faa"))
    with pytest.raises(NameError):
        b.sequenceStats(out, path)


def test_seq_signature_and_read(tmp_path):
    g = gs.GenomicSignatures(4, 1)
    sig = g.seqSignature("ACGTacgtNACGU")
    assert sig.sum() == pytest.approx(1.0) and sig[g.kmerToCanonicalIndex["ACGT"]] == 2 / 5.0
    assert np.isnan(g.seqSignature("ACG")).all()
    text = TETRA["n_runs"]
    p = tmp_path / "t.tsv"
    p.write_text(text)
    got = g.read(str(p))
    assert list(got) == [k for k, _v in BINS["n_runs"]["view"]]
    assert g.distance(got["run9"], got["run9"]) == 0.0


def test_calculate_without_a_device_exits(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    path, out = write_case(tmp_path, BINS["crlf"])
    code = ("import sys, logging\nlogging.basicConfig(stream=sys.stderr)\n"
            "from checkm_amd.binStatistics import BinStatistics\nBinStatistics(1).calculate([%r], %r, 'bin_stats.tsv')\n" % (path, out))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1 and "No usable MI355X" in r.stderr


def test_dropin_rebinds_the_two_classes_when_present(tmp_path):
    pkg = tmp_path / "stand_in" / "checkm"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_module_classes.json")))["classes"]
    for mod, classes in gold.items():
        (pkg / (mod.split(".")[1] + ".py")).write_text("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
    (pkg / "binStatistics.py").write_text("class BinStatistics(object):\n    pass\n")
    (pkg / "genomicSignatures.py").write_text("class GenomicSignatures(object):\n    pass\n")
    code = ("import checkm.binStatistics as b, checkm.genomicSignatures as g\n"
            "import checkm_amd.dropin as d; d.install()\n"
            "assert b.BinStatistics.__module__ == 'checkm_amd.binStatistics', b.BinStatistics.__module__\n"
            "assert g.GenomicSignatures.__module__ == 'checkm_amd.genomicSignatures'\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=str(tmp_path / "stand_in") + os.pathsep + ROOT, CHECKM_DATA_PATH=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-1500:]


def test_empty_bin_logs_and_gets_no_line(caplog):
    st = bs.BinStatistics(1)
    r = dict(count=np.array([[0, 0, 0, 0, 20, 0, 20, 0]], dtype=np.uint64), piece_off=np.array([0, 0], dtype=np.uint64), piece_len=np.zeros(0, dtype=np.uint64))
    with caplog.at_level(logging.ERROR, logger="timestamp"):
        assert st._bin_stats("emptybin", r, 0, 1, (-1, -1, -1)) is None
    assert "emptybin" in caplog.text
