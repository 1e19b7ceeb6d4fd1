"""The nucleotide model scan on the device: the kernels of libcheckm_hip (kernels_nhmm.hip) against the host executor of the same
definition (tests/emu/ssufinder) at == -- every reported row and every hit -- on the smallest shapes that can still break: models
around one node per lane and around a wavefront, at every instance of the kernel and at the cap of 2048 nodes; contigs of no, one and
two bases, shorter than the model, of exactly one tile and one base more; copies at the first and the last base, across a tile
boundary and on the reverse strand; N runs and lower case; hundreds of tiny contigs in one launch; two models in one call; budgets that
force several launches; a threshold of -2^20, so that nearly every row is compared; then SSU_Finder.run on a synthetic data directory."""
import os

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import ssuFinder as sf
from checkm_amd.defaultValues import DefaultValues
from checkm_amd.hmmerModelParser import read_nuc_models
from tests import ssufinder_synth as syn
from tests.emu import ssufinder as emu
from tests.test_ssufinder_host import HIT_F, LOW, ROW_F, read_seqs

pytestmark = pytest.mark.gpu


def same(gpu_ctx, tables, seqs, budget_bytes=0):
    want, got = emu.nhmm_run(None, tables, seqs, budget_bytes), _lib.nhmm_run(gpu_ctx, tables, seqs, budget_bytes)
    for f in ROW_F + HIT_F:
        assert np.array_equal(want[f], got[f]), f
    for f in ("tiles", "launches", "cells", "batches"):
        assert want[f] == got[f], f
    return got


def model(tmp_path, M, seed):
    p = str(tmp_path / ("m%d.hmm" % M))
    cons = syn.write_model(p, "m%d" % M, M, seed)
    return cons, read_nuc_models(p)[0]


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 127, 129, 640, 2048])
def test_rows_and_hits_equal_the_executor(gpu_ctx, tmp_path, M):
    cons, m = model(tmp_path, M, 700 + M)
    rng = np.random.default_rng(M)
    L = max(200, M + 130)
    copy = syn.mutated_copy(rng, cons, clean=min(20, M // 2))
    big, _ = syn.planted_contig(rng, L, [(0, cons, False), (L - M, cons, True)])                 # copies at the first and at the last base
    cross, _ = syn.planted_contig(rng, L, [(max(0, 64 - M // 2), copy, False)])                  # a copy across the first tile boundary
    cross = cross[:100] + "NNNNNnnnnnRY" + cross[112:150].lower() + cross[150:]
    recs = [("empty", ""), ("one", "G"), ("two", "uT"), ("short", syn.random_dna(rng, max(1, M - 1))[:150]), ("tile", syn.random_dna(rng, 64)),
            ("tile1", syn.random_dna(rng, 65)), ("ends", big), ("cross", cross), ("rev", syn.revcomp(cross))]
    seqs = read_seqs(tmp_path, recs)
    got = same(gpu_ctx, _lib.NhmmTables([(m.emis, m.trans)], [LOW], 64, 32, 3), seqs)
    assert len(got["row_pos"]) == 2 * sum(len(s) for _, s in recs) and got["launches"] == 1
    seqs.close()


def test_many_small_contigs_two_models_and_budgets(gpu_ctx, tmp_path):
    (c65, m65), (_, m2), (_, m640) = model(tmp_path, 65, 1), model(tmp_path, 2, 2), model(tmp_path, 640, 3)
    rng = np.random.default_rng(9)
    recs = [("t%03d" % k, syn.random_dna(rng, 10)) for k in range(300)] + [("copy", syn.planted_contig(rng, 400, [(130, c65, False), (260, c65, True)])[0])]
    seqs = read_seqs(tmp_path, recs)
    for strands in (3, 1, 2):
        t = _lib.NhmmTables([(m65.emis, m65.trans), (m2.emis, m2.trans), (m640.emis, m640.trans)], [20000, LOW, 0], 64, 32, strands)
        one = same(gpu_ctx, t, seqs)
        assert one["batches"] == 1 and one["launches"] == 3 and one["tiles"] == 3 * (300 + 7) * (2 if strands == 3 else 1)
        few = same(gpu_ctx, t, seqs, budget_bytes=8 * 1000)
        tiny = same(gpu_ctx, t, seqs, budget_bytes=1)
        assert tiny["batches"] == tiny["tiles"] > few["batches"] > 1
        for f in ROW_F + HIT_F:
            assert np.array_equal(one[f], few[f]) and np.array_equal(one[f], tiny[f])
    hits65 = [(int(one["hit_from"][k]), int(one["hit_to"][k])) for k in range(len(one["hit_model"])) if one["hit_model"][k] == 0]
    assert len(hits65) >= 1
    seqs.close()


def test_the_finders_geometry_at_the_cap(gpu_ctx, tmp_path):
    cons, m = model(tmp_path, 2048, 77)
    rng = np.random.default_rng(78)
    text, where = syn.planted_contig(rng, 16384 + 700, [(15000, syn.mutated_copy(rng, cons), False)])
    seqs = read_seqs(tmp_path, [("long", text), ("exact", syn.random_dna(rng, 300))])
    got = same(gpu_ctx, _lib.NhmmTables([(m.emis, m.trans)], [100000], sf.STRIDE, m.maxl, 3), seqs)
    assert got["tiles"] == 6 and [(int(a), int(b)) for a, b in zip(got["hit_from"], got["hit_to"])] == [(where[0][0], where[0][1])]
    seqs.close()


def test_run_end_to_end(gpu_ctx, tmp_path, monkeypatch):
    root = str(tmp_path / "data")
    cons = syn.data_dir(root)
    monkeypatch.setattr(DefaultValues, "CHECKM_DATA_DIR", root)
    rng = np.random.default_rng(31)
    c1, _ = syn.planted_contig(rng, 900, [(100, syn.mutated_copy(rng, cons["bacteria"]), False), (500, syn.mutated_copy(rng, cons["archaea"]), True)])
    c2, _ = syn.planted_contig(rng, 700, [(300, syn.mutated_copy(rng, cons["euk"]), True)])
    contigs = str(tmp_path / "contigs.fna.gz")
    syn.write_fasta(contigs, [("c1", c1), ("c2 second", c2), ("c3", syn.random_dna(rng, 500))])
    binFile = str(tmp_path / "bin1.fna")
    syn.write_fasta(binFile, [("c1", c1)])
    outs = {}
    for name, engine in (("device", lambda t, s, b=0: _lib.nhmm_run(gpu_ctx, t, s, b)), ("executor", lambda t, s, b=0: emu.nhmm_run(None, t, s, b))):
        monkeypatch.setattr(sf, "_nhmm_run", engine)
        out = str(tmp_path / name)
        sf.SSU_Finder(1).run(contigs, [binFile], out, 1e-5, 200)
        outs[name] = {f: open(os.path.join(out, f)).read() for f in sorted(os.listdir(out))}
    assert outs["device"] == outs["executor"]
    assert sorted(outs["device"]) == ["ssu.archaea.table.txt", "ssu.bacteria.table.txt", "ssu.euk.table.txt", "ssu.fna", "ssu_summary.tsv"]
    rows = outs["device"]["ssu_summary.tsv"].splitlines()[1:]
    assert sorted(r.split("\t")[:3] for r in rows) == [["bin1", "c1", "archaea"], ["bin1", "c1-#1", "bacteria"], ["unbinned", "c2", "euk"]]      # archaea enters first, the relabelling counts from 1
