"""SSU_Finder without a device: the host executor of checkm_amd/csrc/nhmm_dev.h against a brute force that never carries a start, tiles
against the untiled recurrence, recovery of planted copies, the hit rule, the E-value boundary and the two filters, the refusals, the
ABI version, and the post-processing against goldens recorded from the reference's own class (tests/golden/ssufinder_cases.json)."""
import gzip
import json
import logging
import os

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import ssuFinder as sf
from checkm_amd.hmmerModelParser import HmmModelError, NUC_FLOOR, read_nuc_models
from tests import ssufinder_synth as syn
from tests.emu import ssufinder as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssufinder_cases.json")
LOW = -(1 << 20)
ROW_F = ("row_model", "row_seq", "row_strand", "row_pos", "row_start", "row_score")
HIT_F = ("hit_model", "hit_seq", "hit_strand", "hit_from", "hit_to", "hit_score")


def read_seqs(tmp_path, records, name="contigs.fna"):
    p = str(tmp_path / name)
    syn.write_fasta(p, records)
    return _lib.NucSeqs([p])


def same(a, b):
    for f in ROW_F + HIT_F:
        assert np.array_equal(a[f], b[f]), f


def random_tables(rng, M, floors=True):
    e = rng.integers(-3000, 2001, (4, M)).astype(np.int32)
    t = rng.integers(-4000, 1, (7, M)).astype(np.int32)
    if floors:
        e[rng.random((4, M)) < 0.05] = NUC_FLOOR
        t[rng.random((7, M)) < 0.08] = NUC_FLOOR
    return e, t


# ---- the brute force: for every start s a plain DP over the paths that enter at row s; no cell carries a start -----------------------
def brute_rows(e, t, x, tbm):
    """x: codes 0..4 of one strand.  Per row i (1-based) the best score over all starts and the smallest start that reaches it."""
    M, L = e.shape[1], len(x)
    NONE = None
    def plus(a, b):
        return NONE if a is NONE else a + b
    def mx(*v):
        v = [q for q in v if q is not NONE]
        return max(v) if v else NONE
    per_row = [[] for _ in range(L + 1)]
    for s in range(1, L + 1):
        pM, pI, pD = [NONE] * (M + 1), [NONE] * (M + 1), [NONE] * (M + 1)
        for i in range(s, L + 1):
            cM, cI, cD = [NONE] * (M + 1), [NONE] * (M + 1), [NONE] * (M + 1)
            for k in range(1, M + 1):
                z = k - 1
                inn = mx(tbm if i == s else NONE, plus(pM[k - 1], int(t[0, z])), plus(pI[k - 1], int(t[1, z])), plus(pD[k - 1], int(t[2, z])))
                cM[k] = plus(inn, int(e[x[i - 1], z]) if x[i - 1] < 4 else 0)
                cI[k] = mx(plus(pM[k], int(t[3, z])), plus(pI[k], int(t[4, z])))
                cD[k] = mx(plus(cM[k - 1], int(t[5, z])), plus(cD[k - 1], int(t[6, z])))
            r = mx(*cM[1:])
            if r is not NONE:
                per_row[i].append((r, s))
            pM, pI, pD = cM, cI, cD
    out = {}
    for i in range(1, L + 1):
        sc = max(v[0] for v in per_row[i])
        out[i] = (sc, min(v[1] for v in per_row[i] if v[0] == sc))
    return out


CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


def codes(seq, rev):
    c = [CODE.get(ch.upper(), 4) for ch in seq]
    return [3 - v if v < 4 else 4 for v in reversed(c)] if rev else c


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_executor_equals_brute_force(tmp_path, M):
    rng = np.random.default_rng(40 + M)
    letters = "ACGTacgtNnUuRY-"
    recs = [("s%d" % k, "".join(letters[i] for i in rng.integers(0, len(letters), L))) for k, L in enumerate((40, 17, 1, 2, 29))]
    models = [random_tables(rng, M, floors=bool(k)) for k in range(2)]
    seqs = read_seqs(tmp_path, recs)
    got = emu.nhmm_run(None, _lib.NhmmTables(models, [LOW, LOW], 1 << 16, 0, 3), seqs)
    want = []
    for m, (e, t) in enumerate(models):
        for q, (_, s) in enumerate(recs):
            for st in (0, 1):
                for i, (sc, start) in sorted(brute_rows(e, t, codes(s, st), emu.tbm(M)).items()):
                    if sc >= LOW:
                        want.append((m, q, st, i, start, sc))
    have = list(zip(*[got[f].tolist() for f in ROW_F]))
    assert have == want and len(want) > 100
    seqs.close()


@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("ssu_small")
    p = str(d / "m10.hmm")
    cons = syn.write_model(p, "m10", 10, 5)
    return p, cons, read_nuc_models(p)[0]


def test_tiled_equals_untiled(tmp_path, small_model):
    _, cons, m = small_model
    rng = np.random.default_rng(6)
    text, _ = syn.planted_contig(rng, 300, [(60, cons, False), (120, cons, True), (190, syn.mutated_copy(rng, cons, clean=2), False), (0, cons, False), (290, cons, True)])
    seqs = read_seqs(tmp_path, [("a", text), ("b", syn.random_dna(rng, 64)), ("c", syn.random_dna(rng, 65)), ("d", "")])
    whole = emu.nhmm_run(None, _lib.NhmmTables([(m.emis, m.trans)], [LOW], 1 << 16, 0, 3), seqs)
    tiled = emu.nhmm_run(None, _lib.NhmmTables([(m.emis, m.trans)], [LOW], 64, 32, 3), seqs)
    small = emu.nhmm_run(None, _lib.NhmmTables([(m.emis, m.trans)], [LOW], 64, 32, 3), seqs, budget_bytes=1)
    assert (whole["row_pos"] - whole["row_start"]).max() < 32          # no best path spans more than the overlap
    same(whole, tiled)
    same(tiled, small)
    assert tiled["tiles"] == 2 * (5 + 1 + 2) and small["batches"] == small["tiles"] > tiled["batches"] == 1 and len(whole["row_pos"]) == 2 * (300 + 64 + 65)
    seqs.close()


def test_planted_copies_come_back_exactly(tmp_path):
    p = str(tmp_path / "m200.hmm")
    cons = syn.write_model(p, "m200", 200, 11)
    rng = np.random.default_rng(12)
    fwd, rev = syn.mutated_copy(rng, cons), syn.mutated_copy(rng, cons)
    text, where = syn.planted_contig(rng, 3000, [(500, fwd, False), (1003, rev, True)])
    fa = str(tmp_path / "c.fna")
    syn.write_fasta(fa, [("contig", text)])
    old = sf._nhmm_run
    sf._nhmm_run = lambda tables, seqs, budget_bytes=0: emu.nhmm_run(None, tables, seqs, budget_bytes)
    try:
        hits = sf.SSU_Finder(1).scan(p, fa, 1e-5)
    finally:
        sf._nhmm_run = old
    assert sorted((h["start"], h["end"], h["rev"]) for h in hits) == sorted(where) and len(hits) == 2
    assert all(h["seqId"] == "contig" and h["evalue"] <= 1e-5 for h in hits)


def test_hit_rule():
    # groups by start: the highest score, at ties the smallest row
    assert emu.hits_of([(5, 20, 100), (5, 21, 130), (5, 22, 130), (5, 23, 90)], 50) == [(5, 21, 130)]
    # score descending, then start ascending; an overlapping candidate is dropped, a closed interval that only touches counts as overlap
    rows = [(30, 40, 500), (10, 20, 500), (20, 25, 400), (41, 45, 300), (26, 29, 200)]
    assert emu.hits_of(rows, 50) == [(10, 20, 500), (30, 40, 500), (41, 45, 300), (26, 29, 200)]
    # a later, lower candidate inside an accepted one never displaces it; coordinates of the reverse strand are turned round
    assert emu.hits_of([(3, 9, 50), (1, 30, 40)], 30, strand=1) == [(22, 28, 50)]
    assert emu.hits_of([], 10) == []


def test_evalue_boundary_and_filters():
    for evalue, W, mu, lam, N in ((1e-5, 260, 2.0, 0.693, 6000), (1e-2, 1800, -9.5, 0.71, 2 * 64 << 20), (5.0, 40, 0.0, 0.693, 400), (1e-30, 2000, -8.0, 0.69, 10 ** 9)):
        s = sf.min_score_for(evalue, W, mu, lam, N)
        assert sf.evalue_of(s, W, mu, lam, N) <= evalue < sf.evalue_of(s - 1, W, mu, lam, N)
    assert sf.min_score_for(1e300, 260, 2.0, 0.693, 6000) == LOW
    # E <= evalue first, then the printed value: 1.04e-5 prints as 1e-05 but is above the threshold; 0.995e-5 passes both
    h = [dict(evalue=1.04e-5, printed="%.2g" % 1.04e-5), dict(evalue=0.995e-5, printed="%.2g" % 0.995e-5), dict(evalue=1e-5, printed="%.2g" % 1e-5),
         dict(evalue=0.99996e-5, printed="1e-05")]
    assert [x["evalue"] for x in sf.filter_hits(h, 1e-5)] == [0.995e-5, 1e-5, 0.99996e-5]
    assert sf.filter_hits([dict(evalue=1.0e-5, printed="1.1e-05")], 1e-5) == []


def test_refusals(tmp_path, small_model):
    _, _, m = small_model
    ok = lambda **kw: _lib.NhmmTables([(kw.get("e", m.emis), kw.get("t", m.trans))], [kw.get("thr", 0)], kw.get("S", 64), kw.get("O", 32), kw.get("strands", 3))
    for check in (_lib.nhmm_check, emu.nhmm_check):
        check(ok())
        big = (np.zeros((4, 2049), dtype=np.int32), np.zeros((7, 2049), dtype=np.int32))
        for bad, code in ((ok(e=big[0], t=big[1]), -7), (ok(thr=LOW - 1), -7), (ok(S=0), -1), (ok(strands=0), -1), (ok(strands=4), -1), (ok(S=1 << 17, O=1), -7)):
            with pytest.raises(_lib.CkmError) as err:
                check(bad)
            assert err.value.code == code
        for row, col, v, tab in ((0, 3, 2049, "e"), (3, 0, NUC_FLOOR - 1, "e"), (2, 2, 1, "t"), (6, 9, NUC_FLOOR - 1, "t")):
            a = {"e": m.emis.copy(), "t": m.trans.copy()}
            a[tab][row, col] = v
            with pytest.raises(_lib.CkmError) as err:
                check(ok(**a))
            assert err.value.code == -7
        check(ok(thr=LOW))
    p = str(tmp_path / "bad.fna")
    with open(p, "wb") as f:
        f.write(b">fine\nACGT\n>second\nACG\xc3\xa9T\n")
    seqs = _lib.NucSeqs([p])
    with pytest.raises(_lib.CkmError) as err:
        emu.nhmm_run(None, ok(), seqs)
    assert err.value.code == -1 and "second" in str(err.value)
    seqs.close()


def test_model_reader(tmp_path):
    p = str(tmp_path / "m.hmm")
    cons = syn.write_model(p, "mm", 7, 3, with_maxl=False)
    with open(p, "a") as f:
        f.write(syn.model_text("second", "ACGU", maxl=9, alph="RNA", with_compo=False))
    a, b = read_nuc_models(p)
    assert (a.name, a.M, a.maxl, a.mu, a.lam) == ("mm", 7, 14, 2.0, 0.693) and (b.name, b.M, b.maxl) == ("second", 4, 9)
    k = "ACGT".index(cons[2])
    assert a.emis[k, 2] == 1766 and sorted(set(a.emis[:, 2].tolist())) == [-2322, 1766]          # lround(1000 log2(.85 / .25)), log2(.05 / .25)
    assert a.trans[:, 0].tolist() == [NUC_FLOOR, NUC_FLOOR, NUC_FLOOR, -6059, -1322, NUC_FLOOR, NUC_FLOOR]
    assert a.trans[:, 3].tolist() == [-44, -737, -737, -6059, -1322, -6059, -1322]
    assert a.trans[3, 6] == -6059 and a.emis.dtype == np.int32 and a.trans.shape == (7, 7)
    with open(p, "w") as f:
        f.write(syn.model_text("prot", "ACGT", alph="amino"))
    with pytest.raises(HmmModelError):
        read_nuc_models(p)
    with open(p, "w") as f:
        f.write(syn.model_text("long", "A" * 2049))
    with pytest.raises(HmmModelError):
        read_nuc_models(p)


def test_abi_is_12():
    assert _lib.load().ckm_abi_version() == 12 == _lib.ABI_VERSION
    assert {"ckm_nhmm_check", "ckm_nhmm_run", "ckm_nhmm_columns_get", "ckm_nhmm_free"} <= set(_lib.EXPORTS)


# ---- the post-processing against the reference's own class ------------------------------------------------------------------------------
class _Log(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)


def run_golden_case(case, tmp_path):
    """SSU_Finder.run with the recorded hit lists in place of the scan; returns (summary, fna, log lines)."""
    contig = str(tmp_path / case["contig_name"])
    op = gzip.open if contig.endswith(".gz") else open
    with op(contig, "wt") as f:
        f.write(case["contig_text"])
    bins = []
    for name, text in case["bins"]:
        bins.append(str(tmp_path / name))
        with open(bins[-1], "w") as f:
            f.write(text)
    finder = sf.SSU_Finder(1)
    labels = {"bacteria": "bacterial 16S", "archaea": "archaeal 16S", "euk": "eukaryotic 18S"}

    def search(seqs, evalue, prefix):
        found = {}
        for dom in ("bacteria", "archaea", "euk"):
            finder.logger.info("Identifying %s." % labels[dom])
            found[dom] = [dict(seqId=h[0], printed=h[1], start=min(h[2], h[3]), end=max(h[2], h[3]), rev=h[2] > h[3]) for h in case["hits"][dom]]
        return found
    finder._hmmSearch = search
    log = _Log()
    finder.logger.addHandler(log)
    level = finder.logger.level
    finder.logger.setLevel(logging.INFO)
    out = str(tmp_path / "out")
    try:
        finder.run(contig, bins, out, case["evalue"], case["concatenate"])
    finally:
        finder.logger.removeHandler(log)
        finder.logger.setLevel(level)
    return open(os.path.join(out, "ssu_summary.tsv")).read(), open(os.path.join(out, "ssu.fna")).read(), [ln.replace(out, "<out>") for ln in log.lines]


def test_goldens_cover_the_listed_cases():
    names = set(c["name"] for c in golden_cases())
    assert {"concat_inside", "concat_outside", "numbered_names", "substring_ids", "domain_longer_wins", "domain_longer_loses", "reverse_strand", "unbinned",
            "evalue_equal", "gz_contigs"} <= names


@pytest.mark.parametrize("k", range(10))
def test_post_processing_equals_the_reference(tmp_path, k):
    case = golden_cases()[k]
    summary, fna, lines = run_golden_case(case, tmp_path)
    assert summary == case["summary"]
    assert fna == case["fna"]
    assert lines == case["log"]
