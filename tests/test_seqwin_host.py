"""SequenceWindows without a device: the plain-Python restatement (tests/seqwin_reference.py) is pinned to what the reference's own plot
classes handed to their axes (tests/golden/seqwin_cases.json, tools/gen_seqwin_golden.py), and the host executor of the device pass
(tests/emu/seqwin_emu.cpp: seqwin_dev.h's piece logic and outlier_dev.h's distance) plus the library's real host code (reader, layout,
coding bases per window) are compared with the restatement at ==."""
import hashlib
import json
import logging
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import seqWindows as sqw
from tests import seqwin_reference as ref
from tests.emu import seqwin as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "seqwin_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
RUNS = [(c["name"], k) for c in GOLD["cases"] for k in range(len(c["runs"]))]


def write_case(d, case):
    """(fasta path, gff path, tetraSigs) of a golden case under directory d."""
    path = os.path.join(str(d), case["name"] + ".fna")
    open(path, "w").write(case["fasta"])
    gff = os.path.join(str(d), "genes.gff")
    if case["gff"] is not None:
        open(gff, "w").write(case["gff"])
    seqs = ref.read_fasta(case["fasta"])
    with np.errstate(invalid="ignore"):
        sigs = {k: ref.signature(s) for k, s in seqs.items() if k not in case["profile_missing"]}
    assert hashlib.sha256("".join(k + "".join(ref.hexes(v)) for k, v in sigs.items()).encode()).hexdigest() == case["profile_sha256"]
    return path, gff, sigs


def outcome(fn):
    """(result, None) or (None, (type name, args)) of a call that may fail as the reference does."""
    try:
        with np.errstate(invalid="ignore"):
            return fn(), None
    except SystemExit as e:
        return None, ("SystemExit", e.code)
    except (KeyError, ZeroDivisionError) as e:
        return None, (type(e).__name__, [str(a) for a in e.args])


def check_run(case, run, gc, gcp, cd, tdw):
    """The four results (each an outcome()) against one golden run."""
    g = run["gc_plot"]
    assert gc[1] is None and ref.hexes(gc[0][0]) == g["data"]
    if g["seqLens"] is not None:
        assert list(gc[0][1]) == g["seqLens"]
    b = run["gc_bias_plot"]
    if b["error"]:
        assert gcp[1] == (b["error"]["type"], b["error"]["args"])
    else:
        assert gcp[1] is None
        assert [x for v in gcp[0].values() for x in ref.hexes(v[1])] == b["windowGC"] and ref.hexes(v[0] for v in gcp[0].values()) == b["seqGC"]
        assert list(gcp[0].keys()) == list(ref.read_fasta(case["fasta"]).keys())
    c = run["coding_plot"]
    if c["error"] and c["error"]["type"] == "SystemExit":
        assert cd[1] == ("SystemExit", c["error"]["code"])
    elif c["error"]:
        assert cd[1] == (c["error"]["type"], c["error"]["args"])
    else:
        assert cd[1] is None and ref.hexes(cd[0][0]) == c["data"]
        if c["seqLens"] is not None:
            assert list(cd[0][1]) == c["seqLens"]
    t = run["tetra_plot"]
    if t["error"]:
        assert tdw[1] == (t["error"]["type"], t["error"]["args"])
    else:
        assert tdw[1] is None and ref.hexes(tdw[0][0]) == t["data"]
        if t["deltas"] is not None:
            assert ref.hexes(tdw[0][2]) == t["deltas"] and list(tdw[0][1]) == t["seqLens"]


@pytest.mark.parametrize("name,k", RUNS)
def test_restatement_reproduces_the_reference_plots(tmp_path, name, k):
    case, run = CASES[name], CASES[name]["runs"][k]
    _path, _gff, sigs = write_case(tmp_path, case)
    seqs, w = ref.read_fasta(case["fasta"]), run["windowSize"]

    def cd():
        if case["gff"] is None:
            raise SystemExit(1)
        return ref.cd_windows(seqs, case["gff"], w)
    check_run(case, run, outcome(lambda: ref.gc_windows(seqs, w)), outcome(lambda: ref.gc_profile(seqs, w)), outcome(cd), outcome(lambda: ref.td_windows(seqs, sigs, w)))


@pytest.fixture
def host_executor(monkeypatch):
    from checkm_amd import runtime
    monkeypatch.setattr(runtime, "get_ctx", lambda: None)
    monkeypatch.setattr(_lib, "seq_windows", emu.seq_windows)


@pytest.mark.parametrize("name,k", RUNS)
def test_sequence_windows_reproduces_the_reference_plots(tmp_path, host_executor, caplog, name, k):
    case, run = CASES[name], CASES[name]["runs"][k]
    path, gff, sigs = write_case(tmp_path, case)
    w = run["windowSize"]
    s = sqw.SequenceWindows()
    with caplog.at_level(logging.ERROR, logger="timestamp"):
        cd = outcome(lambda: s.cdWindows(path, gff, w))
    if cd[1] and cd[1][0] == "SystemExit":
        assert caplog.records[-1].getMessage() == run["coding_plot"]["error"]["log"][0]
    check_run(case, run, outcome(lambda: s.gcWindows(path, w)), outcome(lambda: s.gcProfile(path, w)), cd, outcome(lambda: s.tdWindows(path, sigs, w)))
    assert s.last_timing["skipped"] == 0 and set(s.last_timing) >= {"read", "copy_in", "count", "td", "copy_out", "coding", "python"}


def random_bin(seed, lens):
    r = random.Random(seed)
    seqs = []
    for n in lens:
        s = [r.choice("ACGT") for _ in range(n)]
        for _ in range(n // 9):
            s[r.randrange(n)] = r.choice("acgtNnUuRY")
        seqs.append("".join(s))
    return seqs


def run_emu(tmp_path, seqs, w, files=1, **kw):
    """The host executor on a bin (or `files` files holding the sequences in turn) with random bin signatures."""
    paths = []
    for f in range(files):
        paths.append(str(tmp_path / ("r%d_%d.fna" % (w, f))))
        open(paths[-1], "w").write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs) if i % files == f))
    b = _lib.NucSeqs(paths)
    try:
        sig = np.random.default_rng(w).random((files, 136))
        sig /= sig.sum(axis=1)[:, None]
        return emu.seq_windows(None, b, w, bin_sig=sig, want_tetra=True, **kw), sig, [b.seq(i).decode() for i in range(b.nseq)], [int(x) for x in b.file_first]
    finally:
        b.close()


def expect(seqs, file_first, sig, w):
    base, tet, td, per_seq = [], [], [], []
    for i, s in enumerate(seqs):
        f = max(k for k in range(len(file_first) - 1) if file_first[k] <= i)
        per_seq.append(ref.base_count(s))
        for win in ref.windows(s, w):
            base.append(ref.base_count(win))
            tet.append(ref.tetra_counts(win))
            with np.errstate(invalid="ignore"):
                td.append(ref.distance(ref.signature(win), sig[f]))
    return base, tet, td, per_seq


def same(r, want):
    base, tet, td, per_seq = want
    assert r["base"].tolist() == [list(x) for x in base] and r["tetra"].tolist() == tet and r["seq"].tolist() == [list(x) for x in per_seq]
    assert ref.hexes(r["td"]) == ref.hexes(td)
    assert r["skipped_seqs"] == 0 and not r["skipped"].any()


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65])
def test_host_executor_equals_the_restatement_on_random_sequences(tmp_path, w):
    lens = [1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20, 31, 33, 63, 64, 65, 66, 127, 128, 129, 130, 131, 195, 200, 257, 1100] + [w, w + 1, 2 * w, 2 * w + 1, 3 * w + 2]
    seqs = random_bin(w, lens)
    want = None
    for piece in (16, 17, 64):
        r, sig, texts, ff = run_emu(tmp_path, seqs, w, files=2, piece_bytes=piece)
        want = want or expect(texts, ff, sig, w)
        same(r, want)
        assert r["first"].tolist() == np.concatenate([[0], np.cumsum([(len(s) - 1) // w if s else 0 for s in texts])]).tolist()
        assert r["pieces"] >= r["windows"]


def test_budget_split_gives_identical_results(tmp_path):
    seqs = random_bin(5, [700, 90, 1500, 64])
    one, sig, texts, ff = run_emu(tmp_path, seqs, 7, piece_bytes=16)
    assert one["batches"] == 1
    b = _lib.NucSeqs([str(tmp_path / "r7_0.fna")])
    try:
        for budget in (544, 544 * 3, 544 * 100):
            r = emu.seq_windows(None, b, 7, bin_sig=sig, piece_bytes=16, budget_bytes=budget)
            assert r["batches"] >= one["windows"] * 544 // budget and r["batches"] > 1
            assert r["base"].tobytes() == one["base"].tobytes() and r["td"].tobytes() == one["td"].tobytes() and r["seq"].tobytes() == one["seq"].tobytes()
        with pytest.raises(_lib.CkmError):                      # the 136 counts of every window do not fit this budget
            emu.seq_windows(None, b, 7, want_tetra=True, budget_bytes=544 * 3)
    finally:
        b.close()
    same(one, expect(texts, ff, sig, 7))


def test_non_ascii_sequences_fall_back_to_python(tmp_path, host_executor, caplog):
    seqs = {"plain": "ACGTTGCAAGCTTCGANNACGTAC", "accent": "ACGTTGéAAGCTTCGATTGACGTAC€GTAACC", "after": "GGCATTACGGATCCA"}
    path = str(tmp_path / "na.fna")
    open(path, "w", encoding="utf-8").write("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    with np.errstate(invalid="ignore"):
        sigs = {k: ref.signature(s) for k, s in seqs.items()}
    s = sqw.SequenceWindows()
    for w in (1, 4, 5, 9):
        with caplog.at_level(logging.DEBUG, logger="timestamp"):
            got = s.tdWindows(path, sigs, w)
        assert s.last_timing["skipped"] == 1 and any("accent" in r.getMessage() for r in caplog.records)
        want = ref.td_windows(seqs, sigs, w)
        assert ref.hexes(got[0]) == ref.hexes(want[0]) and got[1] == want[1] and ref.hexes(got[2]) == ref.hexes(want[2])
        assert ref.hexes(s.gcWindows(path, w)[0]) == ref.hexes(ref.gc_windows(seqs, w)[0])
        (p, perr), (q, qerr) = outcome(lambda: s.gcProfile(path, w)), outcome(lambda: ref.gc_profile(seqs, w))
        assert perr == qerr and (perr is None) == (w > 2)           # w = 1: the windows 'N' and 'é' have no base, as in the reference
        if perr is None:
            assert {k: [v[0].hex(), ref.hexes(v[1])] for k, v in p.items()} == {k: [v[0].hex(), ref.hexes(v[1])] for k, v in q.items()}


@pytest.mark.parametrize("bad", [0, -1, 2.0, "5", None, True, 2 ** 31])
def test_window_size_must_be_a_positive_integer(tmp_path, host_executor, bad):
    path = str(tmp_path / "v.fna")
    open(path, "w").write(">a\nACGTACGT\n")
    s = sqw.SequenceWindows()
    for call in (lambda: s.gcWindows(path, bad), lambda: s.gcProfile(path, bad), lambda: s.cdWindows(path, path, bad), lambda: s.tdWindows(path, {}, bad)):
        with pytest.raises(ValueError):
            call()


def test_layout_and_coding_of_the_library(tmp_path):
    """ckm_seq_windows_layout against (L - 1) // w and ckm_seq_windows_coding against the numpy mask, on every golden case with a GFF."""
    for case in GOLD["cases"]:
        (tmp_path / case["name"]).mkdir()
        path, gff, _sigs = write_case(tmp_path / case["name"], case)
        seqs = ref.read_fasta(case["fasta"])
        b = _lib.NucSeqs([path])
        try:
            for w in sorted(set(case["windows"] + [2, 6, 11])):
                first = _lib.seq_windows_layout(b, w)
                assert np.diff(first).tolist() == [(len(s) - 1) // w if s else 0 for s in seqs.values()]
                coding, missing = _lib.seq_windows_coding(b, [gff], w)
                if case["gff"] is None:
                    assert missing.tolist() == [True] and (coding == -1).all()
                    continue
                masks = ref.coding_masks(case["gff"])
                want = [int(np.sum(masks[k][x * w:(x + 1) * w])) if k in masks else 0 for k, s in seqs.items() for x in range(len(ref.windows(s, w)))]
                assert coding.tolist() == want and missing.tolist() == [False]
            for bad in (0, -3, 2 ** 31):
                with pytest.raises(_lib.CkmError):
                    _lib.seq_windows_layout(b, bad)
        finally:
            b.close()


def test_dropin_routes_the_plot_classes_through_the_library(tmp_path):
    """dropin.install() in a process of its own (tests/seqwin_dropin_driver.py), the device pass on the host executor: the four plot
    classes with recording axes reproduce the goldens, one pass of the library per (file, window size), the fallback counter at 0.  By
    default the plot classes are the project's own stand-ins (tests/seqwin_standin.py), which covers the hook protocol only; the
    reference's unmodified classes run when CHECKM_SOURCE names a CheckM source tree."""
    import subprocess
    import sys
    emu.build()
    cmd = [sys.executable, os.path.join(ROOT, "tests", "seqwin_dropin_driver.py"), "emu", str(tmp_path)]
    if os.path.isdir(os.path.join(os.environ.get("CHECKM_SOURCE", ""), "checkm", "plot")):
        cmd.append(os.environ["CHECKM_SOURCE"])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok 64"), (out.stdout[-500:], out.stderr[-3000:])
