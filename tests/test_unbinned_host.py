"""Unbinned without a device: the full `run` against what the reference's own class wrote, logged and raised
(tests/golden/unbinned_cases.json, tools/gen_unbinned_golden.py) with the device count served by the host executor
(tests/emu/unbinned_emu.cpp: unbinned_dev.h's per-word logic and tile geometry), the host executor against a byte-wise Python
restatement, and the library's real host code: the id reader, the selection and the writer."""
import gzip
import inspect
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import unbinned as ubn
from tests.emu import unbinned as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "unbinned_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}


def write_inputs(d, c):
    """(bin paths, assembly path) of a golden case under directory d, byte for byte."""
    paths = []
    for b in c["bins"]:
        p = os.path.join(str(d), b["name"])
        data = b["text"].encode("utf-8")
        if p.endswith(".gz"):
            with gzip.GzipFile(p, "wb", mtime=0) as g:
                g.write(data)
        else:
            open(p, "wb").write(data)
        paths.append(p)
    asm = os.path.join(str(d), "assembly.fna")
    if c["assembly"] is not None:
        open(asm, "wb").write(c["assembly"].encode("utf-8"))
    return paths, asm


class Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.out = []

    def emit(self, record):
        self.out.append([record.levelname, record.getMessage()])


def read_or_none(p):
    return open(p, "rb").read().decode("utf-8") if os.path.exists(p) else None


def check_case(d, c):
    """Unbinned.run over one golden case: files, log records and failure are the reference's.  Returns the Unbinned."""
    bins, asm = write_inputs(d, c)
    seqOut, statsOut = os.path.join(str(d), "out.fna"), os.path.join(str(d), "out.tsv")
    logger, h = logging.getLogger("timestamp"), Records()
    logger.addHandler(h)
    level = logger.level
    logger.setLevel(logging.INFO)
    error = None
    u = ubn.Unbinned()
    try:
        u.run(bins, asm, seqOut, statsOut, c["minSeqLen"])
    except (ZeroDivisionError, SystemExit) as e:
        error = dict(type=type(e).__name__, message=str(e))
    finally:
        logger.removeHandler(h)
        logger.setLevel(level)
    assert error == c["error"]
    assert read_or_none(seqOut) == c["out_seq"] and read_or_none(statsOut) == c["out_stats"]
    assert [[lvl, m.replace(str(d) + os.sep, "<dir>/")] for lvl, m in h.out] == c["log"]
    return u


@pytest.fixture
def host_executor(monkeypatch):
    from checkm_amd import runtime
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    monkeypatch.setattr(_lib, "unbinned_count", emu.unbinned_count)


def test_the_goldens_hold_the_cases_and_three_kinds_of_failure():
    assert set(CASES) >= {"basic", "repeated", "n_short", "n_long", "utf8", "no_final_newline", "gz_crlf", "min0_empty", "empty_assembly", "all_binned", "missing"}
    assert [CASES[n]["error"]["type"] for n in ("n_long", "min0_empty", "empty_assembly", "no_base")] == ["ZeroDivisionError"] * 4
    assert CASES["n_short"]["error"] is None and ">n\n" not in CASES["n_short"]["out_seq"]
    assert CASES["n_long"]["out_seq"].endswith(">n\nNNNNNNNNNN\n") and CASES["n_long"]["out_stats"].count("\n") == 2
    assert CASES["all_binned"]["out_stats"] == "Sequence Id\tLength\tGC\n" and CASES["all_binned"]["out_seq"] == ""
    assert CASES["empty_assembly"]["out_stats"] == "Sequence Id\tLength\tGC\n"
    assert "u1" not in CASES["utf8"]["out_stats"] and "\nu2\t10\t" in CASES["utf8"]["out_stats"]       # 12 bytes, 9 code points: below 10


@pytest.mark.parametrize("name", list(CASES))
def test_run_reproduces_the_reference(tmp_path, host_executor, name):
    u = check_case(tmp_path, CASES[name])
    if CASES[name]["error"] is None or CASES[name]["error"]["type"] == "ZeroDivisionError":
        assert set(u.last_timing) >= {"read_bins", "read_assembly", "select", "copy_in", "kernel", "copy_out", "write"}


# ---- the host executor against a byte-wise restatement -----------------------------------------------------------------------------------

def base_count(b):
    """baseCount and len() of a sequence given as bytes: upper-cased, T with U, code points = bytes outside 0x80-0xBF."""
    s = bytes(b).upper()
    return [s.count(b"A"), s.count(b"C"), s.count(b"G"), s.count(b"T") + s.count(b"U"), sum(1 for x in s if not 0x80 <= x <= 0xBF)]


def layout(seqs, rng):
    """The reader's layout of byte strings: every sequence at a 16-byte boundary, 64 bytes of slack -- but the padding holds letters and
    other non-zero bytes instead of zeros, so that a count that looks past a sequence's end shows."""
    off, pos = [], 0
    for s in seqs:
        off.append(pos)
        pos += (len(s) + 15) // 16 * 16
    text = rng.choice(np.frombuffer(b"ACGTUacgtu\x80\xc3N", dtype=np.uint8), pos + 64)
    for o, s in zip(off, seqs):
        text[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return text, np.array(off, dtype=np.uint64), np.array([len(s) for s in seqs], dtype=np.uint64)


def random_seq(rng, n):
    """Letters of both cases, N, U, every other byte value now and then."""
    s = rng.choice(np.frombuffer(b"ACGTacgtUuNn", dtype=np.uint8), n)
    wild = rng.random(n) < 0.15
    s[wild] = rng.integers(0, 256, int(wild.sum()), dtype=np.uint8)
    return s.tobytes()


@pytest.mark.parametrize("tile", [16, 48, 64])
def test_host_executor_against_the_restatement(tile):
    rng = np.random.default_rng(tile)
    lens = [0, 1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile + 3] * 2
    seqs = [random_seq(rng, n) for n in lens]
    text, off, nbytes = layout(seqs, rng)
    want = np.array([base_count(s) for s in seqs], dtype=np.uint64)
    n = len(seqs)
    for keep in (np.ones(n, np.uint8), np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), (np.arange(n) % 2 == 0).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)):
        for budget in (1 << 30, 64, 16):
            got, info = emu.count_raw(text, off, nbytes, keep, tile, budget)
            assert got.tolist() == (want * keep[:, None]).tolist()
            tiles = sum(-(-int(L) // tile) for L, k in zip(lens, keep) if k)
            assert int(info[0]) == int(keep.sum()) and int(info[1]) == tiles
            assert int(info[2]) == (tiles if budget == 16 else int(info[2])) and (budget < 1 << 30 or int(info[2]) == (1 if tiles else 0))


def test_every_byte_value_is_classified_as_python_does():
    every = bytes(range(256)) * 2
    text, off, nbytes = layout([every, every[::-1], every[3:]], np.random.default_rng(1))
    got, _info = emu.count_raw(text, off, nbytes, [1, 1, 1], 64, 1 << 20)
    assert got.tolist() == [base_count(every), base_count(every[::-1]), base_count(every[3:])]
    assert base_count(every)[:4] == [4, 4, 4, 8]


# ---- the library's host code -----------------------------------------------------------------------------------------------------------

def test_abi_version_is_unchanged():
    assert _lib.load().ckm_abi_version() == 12


def test_id_reader_equals_the_sequence_reader(tmp_path):
    for c in GOLD["cases"]:
        d = tmp_path / c["name"]
        d.mkdir()
        bins, asm = write_inputs(d, c)
        paths = bins + ([asm] if c["assembly"] is not None else [])
        ids, seqs = _lib.FastaIds(paths), _lib.NucSeqs(paths)
        try:
            assert ids.ids() == seqs.ids() and ids.file_first.tolist() == seqs.file_first.tolist()
            assert ids.seq_bytes.tolist() == seqs.seq_bytes.tolist()
            assert ids.seq_cp.tolist() == [len(seqs.seq(i).decode("utf-8")) for i in range(seqs.nseq)] == _lib.seq_lengths(seqs)
        finally:
            ids.close()
            seqs.close()
    with pytest.raises(_lib.CkmError) as e:
        _lib.FastaIds([str(tmp_path / "absent.fna")])
    assert e.value.code == -2


def test_selection_and_totals(tmp_path):
    c = CASES["basic"]
    bins, asm = write_inputs(tmp_path, c)
    ids, seqs = _lib.FastaIds(bins), _lib.NucSeqs([asm])
    try:
        keep, tot = _lib.unbinned_select(ids, seqs, 5)
        assert seqs.ids() == ["c1", "c2", "c3", "c4", "c5", "c6"] and keep.tolist() == [0, 0, 1, 0, 1, 1]
        assert tot == dict(binned_ids=3, binned_bases=10 + 10 + 10 + 12, all_seqs=6, all_bases=10 + 10 + 16 + 4 + 23 + 6, unbinned_seqs=3, unbinned_bases=16 + 23 + 6)
        assert _lib.unbinned_select(None, seqs, -3)[0].tolist() == [1] * 6
        assert _lib.unbinned_select(ids, None, 0)[1]["binned_ids"] == 3
    finally:
        ids.close()
        seqs.close()


def test_rows_on_rounding_ties_equal_pythons(tmp_path):
    """The writer's %.2f against Python's for the reference's expression, on quotients whose third decimal is a 5 (exact ties in binary,
    such as 1/8 and 1/32, and near ties, such as 1.005 %), and on large counts."""
    pairs = [(1, 8), (3, 8), (1, 32), (3, 32), (1, 160), (3, 160), (201, 20000), (67, 20000), (2001, 200000), (1, 3), (2, 3), (1, 1), (0, 7), (12345678901, 98765432109),
             (2 ** 40 + 1, 2 ** 41 + 3), (1, 2 ** 33), (999, 1000), (9995, 10000), (99995, 100000), (5, 1000), (15, 1000), (25, 1000), (35, 1000), (45, 1000), (1005, 100000)]
    path = str(tmp_path / "a.fna")
    open(path, "w").write("".join(">s%d\nACGTN\n" % k for k in range(len(pairs))))
    seqs = _lib.NucSeqs([path])
    try:
        counts = np.array([[acgt - gc, gc, 0, 0, 5] for gc, acgt in pairs], dtype=np.uint64)
        assert _lib.unbinned_write(seqs, np.ones(len(pairs), np.uint8), counts, str(tmp_path / "o.fna"), str(tmp_path / "o.tsv")) == -1
        want = "Sequence Id\tLength\tGC\n" + "".join("%s\t%d\t%.2f\n" % ("s%d" % k, 5, float(gc) * 100 / acgt) for k, (gc, acgt) in enumerate(pairs))
        assert open(str(tmp_path / "o.tsv")).read() == want
        assert "\t12.50\n" in want or "\t12.5" in want
        # a count that disagrees with the reader's code points is refused, a zero denominator stops the writing and names the sequence
        counts[3, 4] = 6
        with pytest.raises(_lib.CkmError):
            _lib.unbinned_write(seqs, np.ones(len(pairs), np.uint8), counts, str(tmp_path / "o.fna"), str(tmp_path / "o.tsv"))
        counts[3] = [0, 0, 0, 0, 5]
        assert _lib.unbinned_write(seqs, np.ones(len(pairs), np.uint8), counts, str(tmp_path / "o.fna"), str(tmp_path / "o.tsv")) == 3
        assert open(str(tmp_path / "o.tsv")).read() == "".join(want.splitlines(True)[:4]) and open(str(tmp_path / "o.fna")).read() == ">s0\nACGTN\n>s1\nACGTN\n>s2\nACGTN\n>s3\nACGTN\n"
    finally:
        seqs.close()


def test_run_without_a_device_exits(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    bins, asm = write_inputs(tmp_path, CASES["basic"])
    code = ("import sys, logging\nlogging.basicConfig(stream=sys.stderr)\n"
            "from checkm_amd.unbinned import Unbinned\nUnbinned().run(%r, %r, %r, %r, 5)\n" % (bins, asm, str(tmp_path / "o.fna"), str(tmp_path / "o.tsv")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1 and "No usable MI355X" in r.stderr and not os.path.exists(str(tmp_path / "o.fna"))


def test_signature_is_the_references():
    assert list(inspect.signature(ubn.Unbinned.run).parameters) == ["self", "binFiles", "seqFile", "outSeqFile", "outStatsFile", "minSeqLen"]
    assert list(inspect.signature(ubn.Unbinned.__init__).parameters) == ["self"]


def test_dropin_rebinds_unbinned_and_tolerates_its_absence(tmp_path):
    """A stand-in `checkm` package of its own, in a subprocess: with checkm/unbinned.py install() rebinds Unbinned; without it install() passes."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_module_classes.json")))["classes"]
    for present in (True, False):
        pkg = tmp_path / ("stand_in_%d" % present) / "checkm"
        pkg.mkdir(parents=True)
        (pkg / "__init__.py").write_text("")
        for mod, classes in gold.items():
            (pkg / (mod.split(".")[1] + ".py")).write_text("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
        if present:
            (pkg / "unbinned.py").write_text("class Unbinned(object):\n    pass\n")
        code = ("import checkm_amd.dropin as d; d.install()\n"
                "import importlib\n"
                "try:\n"
                "    m = importlib.import_module('checkm.unbinned')\n"
                "except ImportError:\n"
                "    print('absent')\n"
                "else:\n"
                "    assert m.Unbinned.__module__ == 'checkm_amd.unbinned', m.Unbinned.__module__\n"
                "    print('rebound')\n")
        env = dict(os.environ, PYTHONPATH=str(pkg.parent) + os.pathsep + ROOT, CHECKM_DATA_PATH=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == ("rebound" if present else "absent"), out.stderr[-1500:]
