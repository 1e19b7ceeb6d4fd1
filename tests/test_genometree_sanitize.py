"""AddressSanitizer + UBSan over the host code of the genome tree: ckm_gtree_check and the host executor ckm_gtree_host (gtree_host.cpp)
with the encoding, the counts, the distances, the joins and the batch cuts of gtree_dev.h, in a stand-alone program
(tests/native/genometree_host_check.cpp).  The seeded case must give the emulator's merge rows under budgets that cut the call into one
batch per tree, a few and one; damaged calls must be refused or run -- never crash, never read or write outside a buffer.  No device
needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd import _lib
from tests.emu import genometree as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
SYMBOLS = "ARNDCQEGHILKMFPSTWYVarndcqeghilkmfpstwyv-.XBZ*"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("genometree_sanitize")
    exe = str(d / "genometree_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "genometree_host_check.cpp"),
           os.path.join(CSRC, "gtree_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, n, ncols, text, cols, base, model, max_dist, budget, damaged):
    nreps = 0 if cols is None else len(cols)
    words = [n, ncols, nreps, base, model, float(max_dist).hex()] + np.asarray(text).reshape(-1).tolist() + ([] if cols is None else np.asarray(cols).reshape(-1).tolist())
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_seeded_case_batches_and_damaged_calls(harness):
    exe, d = harness
    rng = np.random.RandomState(27)
    n, ncols, nreps = 12, 61, 4
    sym = np.frombuffer(SYMBOLS.encode(), dtype=np.uint8)
    text = sym[rng.randint(0, len(sym), (n, ncols))]
    text[3] = ord("-")
    cols = rng.randint(0, ncols, (nreps, ncols))
    t = _lib.GtreeTables(text=np.ascontiguousarray(text).reshape(-1), nrows=n, ncols=ncols, cols=cols, model="kimura", max_dist=3.0)
    want = emu.gtree_run(None, t, counts=True)
    per_tree = n * 64 + n * n * 16 + n * 64
    for budget, damaged, rounds in ((1, 300, 5), (per_tree * 2, 0, 3), (1 << 30, 0, 1)):
        lines = run(exe, d, n, ncols, text, cols, 1, 0, 3.0, budget, damaged)
        assert lines[0] == "check rc=0"
        assert lines[1] == "counts %d %d" % (want["compared"].sum(), want["differ"].sum())
        rows = [ln.split() for ln in lines if len(ln.split()) == 6 and not ln.startswith(("check", "damaged", "error"))]
        assert [(int(r[0]), int(r[1])) for r in rows] == [(k, r) for k in range(1 + nreps) for r in range(n - 1)]
        assert [[int(r[2]), int(r[3])] for r in rows] == want["merge_ij"].reshape(-1, 2).tolist()
        assert [[float.fromhex(r[4]), float.fromhex(r[5])] for r in rows] == want["merge_len"].reshape(-1, 2).tolist()
        assert int([ln for ln in lines if ln.startswith("rounds ")][0].split()[1]) == rounds
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged rc=0" in codes


def test_refused_calls(harness):
    exe, d = harness
    text = np.full((2, 3), ord("A"), dtype=np.uint8)
    assert run(exe, d, 2, 3, text, None, 1, 0, 3.0, 64, 0)[0] == "check rc=0"
    assert run(exe, d, 2, 3, text, [[0, 1, 3]], 1, 0, 3.0, 64, 0)[0] == "check rc=-1"
    assert run(exe, d, 2, 3, text, None, 1, 3, 3.0, 64, 0)[0] == "check rc=-1"
    assert run(exe, d, 2, 3, text, None, 1, 0, 0.0, 64, 0)[0] == "check rc=-1"
    assert run(exe, d, 2, 3, text, None, 2, 0, 3.0, 64, 0)[0] == "check rc=-1"
    assert run(exe, d, 1, 6, text, None, 1, 0, 3.0, 64, 0)[0] == "check rc=-1"
    bad = text.copy()
    bad[1, 2] = 0x80
    assert run(exe, d, 2, 3, bad, None, 1, 0, 3.0, 64, 0)[0] == "check rc=-7"
    rows = (1 << 14) + 1
    assert run(exe, d, rows, 1, np.full((rows, 1), 65, dtype=np.uint8), None, 1, 0, 3.0, 64, 0)[0] == "check rc=-7"
