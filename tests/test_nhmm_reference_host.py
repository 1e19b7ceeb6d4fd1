"""The independent reference of the nucleotide model scan (tests/nhmm_reference.py) pinned without a device: against the brute force of
tests/test_ssufinder_host.py at M = 1 .. 6, against the host executor on every table family and model size that
tests/test_gpu_nhmm_tables.py puts to the kernel, and the model reader on files whose every node has its own numbers.  The families,
the contigs and the comparisons live here and the device tests import them, so both sides are pinned on the same inputs."""
import math

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.hmmerModelParser import NUC_FLOOR, read_nuc_models
from tests import nhmm_reference as ref
from tests import ssufinder_synth as syn
from tests.emu import ssufinder as emu
from tests.test_ssufinder_host import HIT_F, LOW, ROW_F, brute_rows, codes, random_tables, read_seqs

STRIDE, OVERLAP = 64, 32
LETTERS = "ACGTacgtNnUuRY-"
# one size on each side of every instance boundary of q_of (64 Q nodes, Q = 1 2 4 8 16 24 32) and sizes whose last lane chunks are padding
SIZES = [1, 2, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025, 1500, 1536, 1537, 2047, 2048]
SAT_SIZES = [1024, 1536, 2048]
FAMILIES = ["random", "floors", "highway", "ties", "zeros", "no_transitions"]
SAT_FAMILIES = ["sat_all", "sat_first_half", "sat_second_half"]
THREE_THR = [-9000, -12000, 20000]          # near the median row score of floors 65, random 257 and highway 129 on contigs()
CASES = [(f, M) for f in FAMILIES for M in SIZES] + [(f, M) for f in SAT_FAMILIES for M in SAT_SIZES]


def q_of(M):
    return next(q for q in (1, 2, 4, 8, 16, 24, 32) if q * 64 >= M)


def contigs():
    """Contigs of 1, 63, 64, 65, 128, 129 and 203 bases over LETTERS, one shorter than the overlap, one run of a single base."""
    rng = np.random.default_rng(2024)
    recs = [("n%d" % L, "".join(LETTERS[i] for i in rng.integers(0, len(LETTERS), L))) for L in (1, 63, 64, 65, 128, 129, 203, 20)]
    return recs + [("run", "g" * 70)]


def tables_of(family, M):
    """(emis [4, M], trans [7, M]) of one case, int32, rows of trans in the order MM IM DM MI II MD DD."""
    rng = np.random.default_rng([FAMILIES.index(family) if family in FAMILIES else 10 + SAT_FAMILIES.index(family), M])
    e, t = random_tables(rng, M, floors=family == "floors")
    if family == "floors" and M >= 129:
        Q = q_of(M)
        t[6, M // 3:M // 3 + 3 * Q] = NUC_FLOOR           # tDD: a run of 3 Q nodes holds two whole lane chunks wherever it starts
        t[5, 2 * M // 3:2 * M // 3 + Q + 3] = NUC_FLOOR   # tMD
    elif family == "highway":
        t[[2, 5, 6]] = 0                                  # tDM = tMD = tDD = 0: a match reaches every later node of its row
    elif family == "ties":
        e = (-1000 * rng.integers(0, 2, (4, M))).astype(np.int32)
        t = (-1000 * rng.integers(0, 2, (7, M))).astype(np.int32)
    elif family == "zeros":
        e[:], t[:] = 0, 0
    elif family == "no_transitions":
        t[:] = NUC_FLOOR
    elif family == "sat_all":
        t[6], t[5] = NUC_FLOOR, 0                         # the sum of tDD is M FLOOR <= -2^31
    elif family == "sat_first_half":
        t[6, :M // 2], t[6, M // 2:] = NUC_FLOOR, 0       # the sum of tDD is M / 2 FLOOR <= -2^30
    elif family == "sat_second_half":
        t[6, :M // 2], t[6, M // 2:] = 0, NUC_FLOOR
    return e, t


def same_columns(want, got, what):
    for f in ROW_F + HIT_F:
        assert np.array_equal(np.asarray(want[f], dtype=np.int64), np.asarray(got[f], dtype=np.int64)), (what, f)


def closed_form(family, M, e, recs, out):
    """The literal rows of the two families that have a closed form, for every row of every contig on both strands."""
    n = 0
    for q, (_, s) in enumerate(recs):
        for st in (0, 1):
            x = ref.codes(s, st)
            for i in range(1, len(s) + 1):
                assert (out["row_seq"][n], out["row_strand"][n], out["row_pos"][n]) == (q, st, i)
                if family == "zeros":
                    own = (i - 1) // STRIDE * STRIDE + 1
                    first = own - OVERLAP if own > OVERLAP else 1
                    want = (ref.tbm(M), first if i > first and M >= 2 else i)
                else:
                    want = (ref.tbm(M) + (int(e[x[i - 1]].max()) if x[i - 1] < 4 else 0), i)
                assert (out["row_score"][n], out["row_start"][n]) == want, (q, st, i)
                n += 1
    assert n == len(out["row_pos"])


@pytest.fixture(scope="module")
def contig_seqs(tmp_path_factory):
    recs = contigs()
    seqs = read_seqs(tmp_path_factory.mktemp("nhmm_ref"), recs)
    yield recs, seqs
    seqs.close()


def test_tbm_equals_the_header():
    assert [ref.tbm(M) for M in range(1, 2049)] == [emu.tbm(M) for M in range(1, 2049)]
    assert (ref.tbm(1), ref.tbm(2), ref.tbm(2048)) == (0, -1585, -21001)


def test_hit_rule_equals_the_header():
    rng = np.random.default_rng(5)
    for strand in (0, 1):
        for n in (0, 1, 7, 60):
            rows = [(int(s), int(s + d), int(sc)) for s, d, sc in zip(rng.integers(1, 40, n), rng.integers(0, 12, n), rng.integers(-3, 4, n))]
            assert ref.hits_of(rows, 60, strand) == emu.hits_of(rows, 60, strand)


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_reference_equals_brute_force(M):
    # the inputs of test_ssufinder_host.test_executor_equals_brute_force
    rng = np.random.default_rng(40 + M)
    recs = [("s%d" % k, "".join(LETTERS[i] for i in rng.integers(0, len(LETTERS), L))) for k, L in enumerate((40, 17, 1, 2, 29))]
    models = [random_tables(rng, M, floors=bool(k)) for k in range(2)]
    got = ref.scan(models, [LOW, LOW], 1 << 16, 0, 3, [s for _, s in recs])
    want = []
    for m, (e, t) in enumerate(models):
        for q, (_, s) in enumerate(recs):
            for st in (0, 1):
                for i, (sc, start) in sorted(brute_rows(e, t, codes(s, st), ref.tbm(M)).items()):
                    if sc >= LOW:
                        want.append((m, q, st, i, start, sc))
    assert list(zip(*[got[f].tolist() for f in ROW_F])) == want and len(want) > 100


@pytest.mark.parametrize("family,M", CASES)
def test_reference_equals_the_executor(contig_seqs, family, M):
    recs, seqs = contig_seqs
    e, t = tables_of(family, M)
    want = ref.scan([(e, t)], [LOW], STRIDE, OVERLAP, 3, [s for _, s in recs])
    got = emu.nhmm_run(None, _lib.NhmmTables([(e, t)], [LOW], STRIDE, OVERLAP, 3), seqs)
    same_columns(want, got, "executor")
    assert want["tiles"] == got["tiles"] and len(want["row_pos"]) > 1000
    if family == "ties" and M >= 2:          # one node has one cell per row
        assert 4 * int(want["row_tie"].sum()) >= len(want["row_tie"])
    if family in ("zeros", "no_transitions"):
        closed_form(family, M, e, recs, got)
    if family.startswith("sat"):
        assert int(t[6].astype(np.int64).sum()) <= -(1 << 30)


def test_reference_equals_the_executor_on_three_models(contig_seqs):
    recs, seqs = contig_seqs
    models = [tables_of("floors", 65), tables_of("random", 257), tables_of("highway", 129)]
    for thr, strands in ((THREE_THR, 3), ([-8000, LOW, 30000], 2), ([LOW, LOW, LOW], 1)):
        want = ref.scan(models, thr, STRIDE, OVERLAP, strands, [s for _, s in recs])
        got = emu.nhmm_run(None, _lib.NhmmTables(models, thr, STRIDE, OVERLAP, strands), seqs)
        same_columns(want, got, "executor")
        assert 0 < len(want["row_pos"]) and len(set(want["row_model"].tolist())) == 3


# ---- the reader on a file whose every node has its own numbers ------------------------------------------------------------------------
def _lround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _bits(field, background, top):
    """The printed -ln p of a field as milli-bits of log2(p / background), capped at top; '*' is FLOOR."""
    return NUC_FLOOR if field == "*" else min(top, _lround(1000.0 * math.log2(math.exp(-float(field)) / background)))


@pytest.mark.parametrize("M,star", [(7, 0.0), (7, 0.2), (65, 0.0), (65, 0.1)])
def test_reader_on_per_node_models(tmp_path, M, star):
    p = str(tmp_path / "pn.hmm")
    _, probs = syn.write_model(p, "pn", M, 17 + M, per_node=np.random.default_rng([M, int(100 * star)]), star=star)
    m = read_nuc_models(p)[0]
    mt, tt = probs["match_text"], probs["trans_text"]
    MM, MI, MD, IM, II, DM, DD = range(7)                     # the file's column order
    emis = np.array([[_bits(mt[k][c], 0.25, 2000) for k in range(M)] for c in range(4)], dtype=np.int32)
    trans = np.full((7, M), NUC_FLOOR, dtype=np.int32)
    for k in range(1, M + 1):
        for row, col in ((3, MI), (4, II)):                   # node k's own
            trans[row, k - 1] = _bits(tt[k][col], 1.0, 0)
        for row, col in ((0, MM), (1, IM), (2, DM), (5, MD), (6, DD)):      # into k: node k - 1's, FLOOR at k = 1
            if k > 1:
                trans[row, k - 1] = _bits(tt[k - 1][col], 1.0, 0)
    assert m.M == M and np.array_equal(m.emis, emis) and np.array_equal(m.trans, trans)
    # the file is what the issue asks for: no two of a node's columns alike ('*' apart), '*' entries where asked for
    for k in range(1, M):
        shown = [f for f in tt[k] if f != "*"]
        assert len(set(shown)) == len(shown) and len(set(mt[k - 1]) - {"*"}) == sum(f != "*" for f in mt[k - 1])
    for a, b in ((3, 5), (1, 2), (4, 6)):                     # MI / MD, IM / DM, II / DD as the tables hold them
        live = (trans[a, 1:] != NUC_FLOOR) | (trans[b, 1:] != NUC_FLOOR)
        assert live.any() and (trans[a, 1:][live] != trans[b, 1:][live]).mean() > 0.9
    stars = sum(f == "*" for row in mt for f in row) + sum(f == "*" for row in tt[1:M] for f in row)
    assert (stars > 0) == (star > 0)


def test_default_model_text_is_unchanged():
    # digests of the text as it was before model_text learnt per_node
    import hashlib
    digest = lambda text: hashlib.sha256(text.encode()).hexdigest()
    assert digest(syn.model_text("m", "ACGT")) == "bef77c4336f2ade38cc915e9b6de53c6e66ba89f0d7d8963fb10749a9a7f9f5a"
    assert digest(syn.model_text("second", "ACGU", maxl=9, alph="RNA", with_compo=False)) == "5a4d82f7ace6b4cb802319bee8b3adef08a216c66809a12cb9cbed834617eecb"
