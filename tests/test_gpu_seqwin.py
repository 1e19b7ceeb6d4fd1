"""SequenceWindows on the device: kernels_seqwin.hip against the plain-Python restatement (tests/seqwin_reference.py) and against what the
reference's plot classes handed to their axes (tests/golden/seqwin_cases.json).  Everything is compared at ==; nothing is timed."""
import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import seqWindows as sqw
from tests import seqwin_reference as ref
from tests.test_seqwin_host import CASES, RUNS, check_run, expect, outcome, random_bin, write_case

pytestmark = pytest.mark.gpu


def device(gpu_ctx, tmp_path, seqs, w, files=1, tag="d", **kw):
    """ckm_seq_windows_run on `files` files holding the sequences in turn, with random bin signatures."""
    paths = []
    for f in range(files):
        paths.append(str(tmp_path / ("%s%d_%d.fna" % (tag, w, f))))
        open(paths[-1], "w").write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs) if i % files == f))
    b = _lib.NucSeqs(paths)
    try:
        sig = np.random.default_rng(w).random((files, 136))
        sig /= sig.sum(axis=1)[:, None]
        return _lib.seq_windows(gpu_ctx, b, w, bin_sig=sig, want_tetra=True, **kw), sig, [b.seq(i).decode() for i in range(b.nseq)], [int(x) for x in b.file_first]
    finally:
        b.close()


def same(r, want):
    base, tet, td, per_seq = want
    assert r["base"].tolist() == [list(x) for x in base] and r["seq"].tolist() == [list(x) for x in per_seq]
    assert r["tetra"].tolist() == tet
    assert ref.hexes(r["td"]) == ref.hexes(td)
    assert r["skipped_seqs"] == 0


@pytest.mark.parametrize("name,k", RUNS)
def test_sequence_windows_reproduces_the_reference_plots(gpu_ctx, tmp_path, name, k):
    case, run = CASES[name], CASES[name]["runs"][k]
    path, gff, sigs = write_case(tmp_path, case)
    w = run["windowSize"]
    s = sqw.SequenceWindows()
    check_run(case, run, outcome(lambda: s.gcWindows(path, w)), outcome(lambda: s.gcProfile(path, w)), outcome(lambda: s.cdWindows(path, gff, w)),
              outcome(lambda: s.tdWindows(path, sigs, w)))
    assert s.last_timing["skipped"] == 0


# window size against piece size: one piece, two pieces, three pieces with a last piece of 1, 2 and 3 bytes (4-mers across every piece
# seam are counted once, across a window seam never: the restatement counts inside the slice)
@pytest.mark.parametrize("w,piece", [(16, 16), (32, 16), (33, 16), (34, 16), (35, 16), (1, 16), (3, 16), (4, 16), (100, 4096), (4096, 4096), (5000, 4096), (8195, 4096)])
def test_windows_against_pieces(gpu_ctx, tmp_path, w, piece):
    seqs = random_bin(w + piece, [3 * w + 5, w, w + 1, 2 * w, 2 * w + 1, 1, 7 * w + 3] + ([2500] if w < 100 else []))
    r, sig, texts, ff = device(gpu_ctx, tmp_path, seqs, w, piece_bytes=piece)
    same(r, expect(texts, ff, sig, w))
    assert r["pieces"] >= r["windows"] * -(-w // piece)


@pytest.mark.parametrize("nseq", [1, 63, 64, 65])
def test_sequence_counts(gpu_ctx, tmp_path, nseq):
    seqs = random_bin(nseq, [20 + (7 * i) % 23 for i in range(nseq)])
    r, sig, texts, ff = device(gpu_ctx, tmp_path, seqs, 9, files=min(3, nseq), tag="n%d_" % nseq)
    same(r, expect(texts, ff, sig, 9))


@pytest.mark.parametrize("nwin", [1, 7, 8, 9, 65])
def test_window_counts_fill_the_td_wavefront_raggedly(gpu_ctx, tmp_path, nwin):
    seqs = random_bin(nwin, [nwin * 11 + 1])
    r, sig, texts, ff = device(gpu_ctx, tmp_path, seqs, 11, tag="k%d_" % nwin)
    assert r["windows"] == nwin
    same(r, expect(texts, ff, sig, 11))


def test_budget_splits_one_sequence_and_two_calls_agree(gpu_ctx, tmp_path):
    seqs = random_bin(77, [900, 40, 2100])
    one, sig, texts, ff = device(gpu_ctx, tmp_path, seqs, 13, piece_bytes=16)
    again, _sig, _t, _f = device(gpu_ctx, tmp_path, seqs, 13, piece_bytes=16)
    same(one, expect(texts, ff, sig, 13))
    assert one["batches"] == 1
    for key in ("base", "seq", "td", "tetra"):
        assert one[key].tobytes() == again[key].tobytes()
    b = _lib.NucSeqs([str(tmp_path / "d13_0.fna")])
    try:
        for budget in (544, 544 * 5, 544 * 64):
            r = _lib.seq_windows(gpu_ctx, b, 13, bin_sig=sig, piece_bytes=16, budget_bytes=budget)
            assert r["batches"] > 1
            assert r["base"].tobytes() == one["base"].tobytes() and r["td"].tobytes() == one["td"].tobytes() and r["seq"].tobytes() == one["seq"].tobytes()
        with pytest.raises(_lib.CkmError):
            _lib.seq_windows(gpu_ctx, b, 13, want_tetra=True, budget_bytes=544 * 5)
    finally:
        b.close()
    assert one["tetra"].sum(axis=1).tolist() == [sum(ref.tetra_counts(win)) for s in texts for win in ref.windows(s, 13)]


def test_dropin_routes_the_plot_classes_through_the_device(tmp_path):
    """The drop-in end to end in a process of its own (tests/seqwin_dropin_driver.py): after dropin.install() the four plot classes with
    recording axes reproduce the goldens from the device pass, one pass per (file, window size), the fallback counter at 0.  By default
    the plot classes are the project's own stand-ins (tests/seqwin_standin.py), which covers the hook protocol only; the reference's
    unmodified classes run when CHECKM_SOURCE names a CheckM source tree."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "seqwin_dropin_driver.py"), "gpu", str(tmp_path)]
    if os.path.isdir(os.path.join(os.environ.get("CHECKM_SOURCE", ""), "checkm", "plot")):
        cmd.append(os.environ["CHECKM_SOURCE"])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok 64"), (out.stdout[-500:], out.stderr[-3000:])
