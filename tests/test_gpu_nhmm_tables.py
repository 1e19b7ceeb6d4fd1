"""nhmm_scan_kernel<Q> (checkm_amd/csrc/kernels_nhmm.hip) on tables that differ at every node: every reported row and every hit of the
device against the independent reference (tests/nhmm_reference.py: int64, no saturation, a closed-form D row, its own tBM, tiles and hit
rule) and against the host executor, at ==.  The models of tests/test_gpu_ssufinder.py repeat one transition column at every node, with
MI = MD, IM = DM and II = DD and no '*'; here the tables are arrays: random per node, with floors and runs of floors over whole lane
chunks, sums of tDD beyond the saturation point of the delete scan, delete highways across all lanes, scores from two values so that
equal scores with different starts are the rule, and two families whose rows are known in closed form.  Model sizes sit on both sides of
every instance boundary and leave padding inside and after lane chunks; the contigs are short (tests/test_nhmm_reference_host.py, which
pins the same reference against the executor on the same cases without a device)."""
import numpy as np
import pytest

from checkm_amd import _lib
from tests import nhmm_reference as ref
from tests.emu import ssufinder as emu
from tests.test_nhmm_reference_host import CASES, OVERLAP, STRIDE, THREE_THR, closed_form, contigs, same_columns, tables_of
from tests.test_ssufinder_host import HIT_F, LOW, ROW_F, read_seqs

pytestmark = pytest.mark.gpu
INFO_F = ("tiles", "launches", "cells", "batches")


@pytest.fixture(scope="module")
def contig_seqs(tmp_path_factory):
    recs = contigs()
    seqs = read_seqs(tmp_path_factory.mktemp("nhmm_tables"), recs)
    yield recs, seqs
    seqs.close()


def three_way(gpu_ctx, models, thr, strands, recs, seqs, budget_bytes=0, want=None):
    """device == reference and device == executor on every column, device == executor on the call's counters; returns (reference, device)."""
    tables = _lib.NhmmTables(models, thr, STRIDE, OVERLAP, strands)
    got = _lib.nhmm_run(gpu_ctx, tables, seqs, budget_bytes)
    want = want or ref.scan(models, thr, STRIDE, OVERLAP, strands, [s for _, s in recs])
    host = emu.nhmm_run(None, tables, seqs, budget_bytes)
    same_columns(want, got, "reference")
    same_columns(host, got, "executor")
    for f in INFO_F:
        assert host[f] == got[f], f
    assert want["tiles"] == got["tiles"]
    return want, got


@pytest.mark.parametrize("family,M", CASES)
def test_kernel_equals_the_reference(gpu_ctx, contig_seqs, family, M):
    recs, seqs = contig_seqs
    e, t = tables_of(family, M)
    want = ref.scan([(e, t)], [LOW], STRIDE, OVERLAP, 3, [s for _, s in recs])
    if family == "ties" and M >= 2:          # a condition on the inputs: with one node a row has one cell
        assert 4 * int(want["row_tie"].sum()) >= len(want["row_tie"])
    if family.startswith("sat"):
        assert int(t[6].astype(np.int64).sum()) <= -(1 << 30)
    _, got = three_way(gpu_ctx, [(e, t)], [LOW], 3, recs, seqs, want=want)
    assert got["launches"] == 1 and len(got["row_pos"]) > 1000
    if family in ("zeros", "no_transitions"):
        closed_form(family, M, e, recs, got)


def three_models():
    return [tables_of("floors", 65), tables_of("random", 257), tables_of("highway", 129)]          # Q = 2, 8 and 4


def test_three_models_of_different_q_in_one_call(gpu_ctx, contig_seqs):
    recs, seqs = contig_seqs
    for thr, strands in ((THREE_THR, 3), ([-8000, LOW, 30000], 2), ([LOW, LOW, LOW], 1)):
        want, got = three_way(gpu_ctx, three_models(), thr, strands, recs, seqs)
        per_launch = got["tiles"] // 3
        assert got["launches"] == 3 and got["batches"] == 1 and got["tiles"] == 3 * per_launch and per_launch % 4 != 0
        assert sorted(set(got["row_model"].tolist())) == [0, 1, 2] and len(got["hit_model"]) > 0


def test_budgets_give_the_same_columns(gpu_ctx, contig_seqs):
    recs, seqs = contig_seqs
    _, whole = three_way(gpu_ctx, three_models(), THREE_THR, 3, recs, seqs)
    _, few = three_way(gpu_ctx, three_models(), THREE_THR, 3, recs, seqs, budget_bytes=8000)
    _, one = three_way(gpu_ctx, three_models(), THREE_THR, 3, recs, seqs, budget_bytes=1)
    assert one["batches"] == one["tiles"] > few["batches"] > whole["batches"] == 1
    for f in ROW_F + HIT_F:
        assert np.array_equal(whole[f], few[f]) and np.array_equal(whole[f], one[f]), f


def test_threshold_at_the_median_row_score(gpu_ctx, contig_seqs):
    """The threshold comes from the reference's scores; rows at the threshold are reported, the scan kernel's count and the fill kernel's
    keep agree there (the number of reported rows is the reference's), and one milli-bit higher those rows are gone."""
    recs, seqs = contig_seqs
    models = three_models()
    texts = [s for _, s in recs]
    every = ref.scan(models, [LOW] * 3, STRIDE, OVERLAP, 3, texts)
    thr = [int(np.sort(every["row_score"][every["row_model"] == m])[int((every["row_model"] == m).sum()) // 2]) for m in range(3)]
    for step in (0, 1):
        at = [v + step for v in thr]
        want, got = three_way(gpu_ctx, models, at, 3, recs, seqs)
        assert len(got["row_pos"]) == len(want["row_pos"]) == sum(int(((every["row_model"] == m) & (every["row_score"] >= at[m])).sum()) for m in range(3))
        for m in range(3):
            on = int(((got["row_model"] == m) & (got["row_score"] == thr[m])).sum())
            assert on == (0 if step else int(((every["row_model"] == m) & (every["row_score"] == thr[m])).sum())) and (step or on > 0)
