"""AddressSanitizer + UBSan over the host code of the near-identity pass: ckm_nearid_check and the host executor ckm_nearid_host
(nearid_host.cpp) with the check, the word arithmetic and the band cuts of nearid_dev.h, in a stand-alone program
(tests/native/nearid_host_check.cpp).  The seeded alignment must give the emulator's bit rows under budgets that cut the call into one
band per row tile, two bands and one; damaged calls -- fewer rows, strides that are no multiple of 16 or below the row length, rows
without a column, limits of 0, any bytes in the text -- must be refused or run: never crash, never read or write outside a buffer.  No
device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd import _lib
from tests import reducedtree_synth as synth
from tests.emu import nearid as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("reducedtree_sanitize")
    exe = str(d / "nearid_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "nearid_host_check.cpp"), os.path.join(CSRC, "nearid_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, n_rows, row_len, row_stride, limit, text, budget, damaged):
    words = [n_rows, row_len, row_stride] + list(limit) + np.asarray(text, dtype=np.uint8).reshape(-1).tolist()
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(int(w)) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_seeded_alignment_bands_and_damaged_calls(harness):
    exe, d = harness
    text = synth.alignment(71, 130, 300, clade=40)
    text[7, 299] = 0xFF
    text[8] = text[7]
    text[8, 299] = 0x7F                                                                # a pair that differs in bit 7 of the last column alone
    limit = np.full(130, emu.limit_of(300), dtype=np.uint32)
    limit[::3] = 1
    limit[5] = 400                                                                     # above the row length: every later row is near
    t = _lib.NearidTables(text, limit)
    want = emu.near_bits(text, limit)
    assert want[5, 0] == np.uint64(0xFFFFFFFFFFFFFFC0) and want.any(axis=1).sum() > 20
    fixed, per = t.n_rows * t.row_stride + t.n_rows * 4, 64 * t.words * 8
    budgets = ((1, 300), (fixed + 2 * per, 0), (1 << 30, 0))
    assert [len(emu.bands(t.n_rows, t.row_stride, b)) for b, _ in budgets] == [3, 2, 1]
    for budget, damaged in budgets:
        lines = run(exe, d, t.n_rows, t.row_len, t.row_stride, t.limit, t.text, budget, damaged)
        assert lines[0] == "check rc=0"
        got = [[int(x, 16) for x in ln.split()[2:]] for ln in lines if ln.startswith("w ")]
        assert got == want.tolist()
        assert int([ln for ln in lines if ln.startswith("bands ")][0].split()[1]) == len(emu.bands(t.n_rows, t.row_stride, budget))
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1"}
        if damaged:
            assert codes.count("damaged rc=-1") > 20 and codes.count("damaged rc=0") > 20


def test_refused_calls(harness):
    exe, d = harness
    text = np.zeros((3, 32), dtype=np.uint8)

    def first_line(n_rows=3, row_len=20, row_stride=32, limit=(1, 1, 1)):
        return run(exe, d, n_rows, row_len, row_stride, limit, text.reshape(-1)[:n_rows * row_stride], 0, 0)[0]

    assert first_line() == "check rc=0"
    assert first_line(n_rows=0, limit=()) == "check rc=-1"
    assert first_line(row_len=0) == "check rc=-1"
    assert first_line(limit=(1, 0, 1)) == "check rc=-1"
    assert first_line(row_len=20, row_stride=16) == "check rc=-1"
    assert first_line(row_len=20, row_stride=24) == "check rc=-1"
    assert first_line(row_len=32) == "check rc=0"
