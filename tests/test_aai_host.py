"""AminoAcidIdentity without a device: the full `run` against what the reference's own class computed, wrote, logged and raised
(tests/golden/aai_cases.json, tools/gen_aai_golden.py) with `_lib.aai_pairs` served by the host executor (tests/emu/aai_emu.cpp:
aai_dev.h's per-chunk logic, pair decode, packing and batches), the host executor against a plain restatement of aai() on the
synthetic set the device tests use, the pair decode, and the library's argument tests.  Everything is compared at ==."""
import ctypes as C
import inspect
import json
import logging
import os

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import aminoAcidIdentity as aam
from tests.emu import aai as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "aai_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
TIMING_KEYS = {"list", "read", "pack", "copy_in", "kernel", "copy_out", "python", "groups", "pairs", "batches"}
# (groups, pairs) that the library takes per case: the groups in front of a failing one, and none that runs the host loop
TAKES = {"empty_tree": (0, 0), "nothing_to_compare": (0, 0), "basic": (3, 5), "column_zero": (6, 14), "ids": (2, 6), "names_and_case": (3, 5), "unequal": (1, 1),
         "owners": (1, 1), "non_ascii": (2, 2), "no_report": (1, 3)}


def write_tree(d, c):
    """The output directory of a golden case under directory d, byte for byte."""
    d = str(d)
    os.makedirs(os.path.join(d, "bins"))
    for b in c["bins"]:
        os.makedirs(os.path.join(d, "bins", b))
    for rel, text in c["files"].items():
        p = os.path.join(d, *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "wb").write(text.encode("utf-8"))
    return d


class Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.out = []

    def emit(self, record):
        self.out.append([record.levelname, record.getMessage()])


def plain(x):
    return {k: (plain(v) if isinstance(v, dict) else v) for k, v in x.items()}


def check_case(d, c, monkeypatch):
    """AminoAcidIdentity.run over one golden case, os.listdir returning sorted names as it did for the reference: scores, summary,
    report bytes, log records and failure are the reference's.  Returns the AminoAcidIdentity."""
    d = write_tree(d, c)
    listdir = os.listdir
    monkeypatch.setattr(os, "listdir", lambda p: sorted(listdir(p)))
    path = os.path.join(d, "alignments.txt") if c["report"] else None
    logger, h = logging.getLogger("timestamp"), Records()
    logger.addHandler(h)
    level = logger.level
    logger.setLevel(logging.INFO)
    error = None
    a = aam.AminoAcidIdentity()
    try:
        a.run(c["threshold"], d, path)
    except (AssertionError, SystemExit) as e:
        error = dict(type=type(e).__name__, message=str(e))
    finally:
        logger.removeHandler(h)
        logger.setLevel(level)
    assert error == c["error"]
    assert plain(a.aaiRawScores) == c["raw"] and plain(a.aaiHetero) == c["hetero"] and plain(a.aaiMeanBinHetero) == c["mean"]
    assert [list(m) for m in a.aaiRawScores.values()] == [list(m) for m in c["raw"].values()] and list(a.aaiRawScores) == list(c["raw"])
    assert (open(path, "rb").read().decode("utf-8") if path and os.path.exists(path) else None) == c["report_text"]
    assert h.out == c["log"]
    return a


@pytest.fixture
def host_executor(monkeypatch):
    from checkm_amd import runtime
    calls = []

    def served(ctx, groups, budget_bytes=0):
        calls.append(len(groups))
        return emu.aai_pairs(ctx, groups, budget_bytes)
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    monkeypatch.setattr(_lib, "aai_pairs", served, raising=True)
    return calls


def test_the_goldens_hold_the_cases_and_both_failures():
    assert list(CASES) == ["empty_tree", "nothing_to_compare", "basic", "column_zero", "ids", "names_and_case", "unequal", "owners", "non_ascii", "no_report"]
    assert CASES["unequal"]["error"] == dict(type="AssertionError", message="") and CASES["unequal"]["report_text"].count("AAI:") == 2
    assert CASES["owners"]["error"] == dict(type="SystemExit", message="1") and CASES["owners"]["log"][-1] == ["ERROR", "Bin ids do not match."]
    assert CASES["owners"]["report_text"].count("AAI:") == 2 and "b2" not in CASES["owners"]["raw"]
    assert CASES["empty_tree"]["raw"] == {} and CASES["nothing_to_compare"]["raw"] == {} and CASES["nothing_to_compare"]["report_text"] == ""
    assert set(CASES["ids"]["raw"]) == {"b1", "solo"} and len(CASES["ids"]["raw"]["b1"]["PF1"]) == 3          # 'solox'[:-1]; the repeated id is one copy
    assert list(CASES["names_and_case"]["raw"]["b1"]) == ["PF00318", "TIGR1"] and len(CASES["names_and_case"]["raw"]["b1"]["PF00318"]) == 4
    assert CASES["names_and_case"]["raw"]["b1"]["PF00318"][1] == 0.0                                          # lower case against upper case
    assert CASES["column_zero"]["raw"]["b1"]["A"] == [1.0, 0.0, 0.0] and CASES["column_zero"]["raw"]["b1"]["D"] == [0.0]
    assert CASES["no_report"]["report_text"] is None


@pytest.mark.parametrize("name", list(CASES))
def test_run_reproduces_the_reference(tmp_path, host_executor, monkeypatch, name):
    c = CASES[name]
    a = check_case(tmp_path, c, monkeypatch)
    assert set(a.last_timing) >= TIMING_KEYS
    takes = TAKES[name]
    assert (a.last_timing["groups"], a.last_timing["pairs"]) == takes            # the groups in front of a failing one still went through the library
    assert host_executor == ([takes[0]] if takes[0] else [])                     # all of them in ONE call
    assert a.last_timing["batches"] == (1 if takes[0] else 0)


def test_without_a_device_run_uses_the_host_loop_and_says_so(tmp_path, monkeypatch):
    from checkm_amd import runtime

    def no_device():
        raise _lib.CkmError(-4, "no HIP device visible")
    monkeypatch.setattr(runtime, "get_ctx", no_device)
    c = dict(CASES["basic"])
    c["log"] = c["log"] + [["WARNING", "No usable MI355X (gfx950) device: the amino-acid identities are computed by the host loop."]]
    a = check_case(tmp_path, c, monkeypatch)
    assert a.last_timing["pairs"] == 0 and a.last_timing["batches"] == 0


def test_signature_and_public_methods_are_the_references():
    assert list(inspect.signature(aam.AminoAcidIdentity.run).parameters) == ["self", "aaiStrainThreshold", "outDir", "alignmentOutputFile"]
    a = aam.AminoAcidIdentity()
    assert a.aai("-A-CD-", "-AC-DE") == 0.5 and a.aai("", "") == 0.0 and a.last_timing == {}
    assert "plain host arithmetic" not in aam.__doc__.lower()


# ---- the host executor against a plain restatement of aai() -----------------------------------------------------------------------------

def aai_plain(x, y):
    """(mismatches, compared, aai) of two rows of bytes of equal length: checkm/aminoAcidIdentity.py:127-161 restated."""
    L = len(x)
    gapped = [x[c] == 45 or y[c] == 45 for c in range(L)]
    start = 0
    while start < L and gapped[start]:
        start += 1
    end = L
    for c in range(L - 1, 0, -1):
        if not gapped[c]:
            break
        end = c
    mis = seqLen = 0
    for c in range(start, end):
        if x[c] != y[c]:
            mis += 1
            seqLen += 1
        elif x[c] != 45:
            seqLen += 1
    return mis, seqLen, (1.0 - (float(mis) / seqLen) if seqLen else 0.0)


LENS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096]
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def pattern_rows(L, rng):
    """The gap patterns at one row length: every pair of these rows is compared."""
    base = rng.choice(LETTERS, L)
    gap = ord("-")

    def made(f):
        r = base.copy()
        f(r)
        return r.tobytes()

    def lead(n):
        return lambda r: r.__setitem__(slice(0, n), gap)

    def trail(n):
        return lambda r: r.__setitem__(slice(n, None), gap)

    def inside(step, shift):
        return lambda r: r.__setitem__(slice(2 + shift, max(2 + shift, L - 2), step), gap)

    def lowered(r):
        if L:
            r[L // 2] |= 0x20
    return [made(lambda r: None),                      # none gapped
            made(lead(L)),                             # all gapped
            made(trail(1)),                            # only column 0 ungapped
            made(lead(1)),                             # only column 0 gapped
            made(lead(16)), made(lead(64)),            # a leading run that ends at 15 | 16 and at 63 | 64
            made(trail(16)), made(trail(64)),          # a trailing run that starts there
            made(inside(3, 0)), made(inside(6, 0)),    # both rows gapped in every sixth column, one of them in every third
            made(inside(5, 1)),                        # a residue against a gap inside
            made(lowered),                             # a single case difference
            made(lambda r: None)]                      # identical rows


def big_rows(n, L, rng):
    rows = rng.choice(np.frombuffer(b"ACDE-", dtype=np.uint8), (n, L), p=[0.3, 0.2, 0.15, 0.1, 0.25])
    return [r.tobytes() for r in rows]


_SYNTH = {}


def synthetic():
    """(groups, expected [npairs, 3] as (mismatches, compared, aai) lists) -- the restatement, computed once per process.  Group sizes 0,
    1, 2, 3, 13, 64, 65 and 300 (44 850 pairs at L = 7), the empty and single-row groups in between, so that pair_off repeats."""
    if not _SYNTH:
        rng = np.random.default_rng(16)
        groups = [[], [b"ACD"]]
        for L in LENS:
            groups += [pattern_rows(L, rng), [], [b"-" * L]]
        groups += [big_rows(2, 33, rng), [], [], big_rows(3, 1, rng), big_rows(64, 33, rng), [b""], big_rows(65, 17, rng), [], big_rows(300, 7, rng), [], [b"A"]]
        want = [aai_plain(g[i], g[j]) for g in groups for i in range(len(g)) for j in range(i + 1, len(g))]
        _SYNTH.update(groups=groups, want=want)
    return _SYNTH["groups"], _SYNTH["want"]


def equals(r, want):
    """mismatches, compared and the bits of aai of a result dict against the restatement."""
    return (r["mismatches"].tolist() == [w[0] for w in want] and r["compared"].tolist() == [w[1] for w in want] and
            r["aai"].tobytes() == np.array([w[2] for w in want], dtype=np.float64).tobytes())


def test_restatement_is_aai():
    a = aam.AminoAcidIdentity()
    for g in synthetic()[0][2:2 + 3 * 7:3]:
        for i in range(len(g)):
            for j in range(i + 1, len(g)):
                assert aai_plain(g[i], g[j])[2] == a.aai(g[i].decode(), g[j].decode())


def test_host_executor_against_the_restatement():
    groups, want = synthetic()
    sizes = [len(g) for g in groups]
    assert {0, 1, 2, 3, 64, 65, 300} <= set(sizes) and len(want) > 44850
    one = emu.aai_pairs(None, groups, budget_bytes=1 << 30)
    assert equals(one, want) and one["nbatches"] == 1
    assert one["pair_off"].tolist() == np.concatenate([[0], np.cumsum([n * (n - 1) // 2 for n in sizes])]).tolist()
    assert (np.diff(one["pair_off"].astype(np.int64)) == 0).sum() >= 20
    cut = emu.aai_pairs(None, groups, budget_bytes=(one["bytes"] + 16 * len(want)) // 3)
    assert equals(cut, want) and cut["nbatches"] >= 3
    tiny = emu.aai_pairs(None, groups[-12:], budget_bytes=1)          # a budget below one group's text: batches of the minimum size
    assert equals(tiny, want[len(want) - tiny["npairs"]:]) and tiny["nbatches"] > 700


def test_pair_decode_is_exact():
    for n in (2, 3, 4, 5, 64, 65, 300):
        k = 0
        for i in range(n):
            for j in range(i + 1, n):
                assert emu.decode(k, n) == (i, j)
                k += 1
    for n in (1 << 20, (1 << 20) - 1, 94907, 3037000):                 # up to and beyond the rows a group may have
        before = lambda i: i * (2 * n - i - 1) // 2
        for i in (0, 1, 2, n // 3, n // 2, n - 3, n - 2):
            assert emu.decode(before(i), n) == (i, i + 1) and emu.decode(before(i + 1) - 1, n) == (i, n - 1)
            if i:
                assert emu.decode(before(i) - 1, n) == (i - 1, n - 1)


# ---- the library's host code -------------------------------------------------------------------------------------------------------------

def test_abi_stays_12_and_the_new_names_are_exported():
    L = _lib.load()
    assert L.ckm_abi_version() == 12
    for name in ("ckm_aai_check", "ckm_aai_run", "ckm_aai_columns_get", "ckm_aai_free"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    assert "#define CKM_ABI_VERSION 12" in header and "ckm_aai_columns;" in header


def test_check_refuses_malformed_input():
    L = _lib.load()

    def rc(gro, ro, text=b"x" * 10000):
        g, r = np.array(gro, dtype=np.uint64), np.array(ro, dtype=np.uint64)
        return L.ckm_aai_check(len(g) - 1, g.ctypes.data, r.ctypes.data, text)
    assert rc([0, 2, 2, 3], [0, 5, 10, 10]) == 0 and rc([0], [0]) == 0 and rc([0, 2], [0, 4096, 8192]) == 0 and rc([0, 2], [0, 0, 0], None) == 0
    assert rc([0, 3], [0, 5, 10, 14]) == -1 and "unequal" in L.ckm_last_error().decode()        # unequal rows in a group
    assert rc([0, 2, 5], [0, 4, 8, 11, 14, 16]) == -1                                          # ... in the second group
    assert rc([0, 2], [0, 4097, 8194]) == -7 and rc([0, 1], [0, 4097]) == -7                   # a row beyond the model limit
    assert rc([0, 2, 1, 3], [0, 5, 10, 15]) == -1 and rc([1, 2], [0, 5, 10]) == -1             # group offsets out of order
    assert rc([0, 2], [0, 5, 4]) == -1 and rc([0, 2], [1, 5, 9]) == -1                         # row offsets out of order
    assert rc([0, 2], [0, 5, 10], None) == -1
    assert L.ckm_aai_check(1, None, None, None) == -1
    out = C.c_void_p()
    g, r = np.array([0, 2], dtype=np.uint64), np.array([0, 3, 7], dtype=np.uint64)
    assert L.ckm_aai_run(None, 1, g.ctypes.data, r.ctypes.data, b"abcdefg", 0, C.byref(out)) == -1
    for groups, code in (([[b"AC", b"A"]], -1), ([[b"A" * 4097] * 2], -7)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.aai_check(groups)
        assert e.value.code == code
    _lib.aai_check([[b"AC", b"AD"], [], ["AC"]])
