"""AddressSanitizer + UBSan over the host code of MarkerSetBuilder: ckm_mset_check (markerset_host.cpp) and the packing, the rounds, the
tile lists, the batch cuts and the per-pair step of markerset_dev.h, in a stand-alone program (tests/native/markerset_host_check.cpp).
The seeded synthetic table must give the plain restatement's pairs under budgets that cut the work into many rounds and batches; damaged
tables must be refused or walked -- never crash, never read or write outside a buffer.  No device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_markerset_host import plain_colocated, plain_markers, synthetic_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("markerset_sanitize")
    exe = str(d / "markerset_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "markerset_host_check.cpp"),
           os.path.join(CSRC, "markerset_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, table, glists, mlists, tU, tS, D, thr, budget, damaged):
    cls, pos_off, pos = table
    words = [cls.shape[0], cls.shape[1], len(glists), repr(float(D)), repr(float(thr))] + cls.reshape(-1).tolist() + pos_off.tolist() + pos.tolist()
    for g, m, u, s in zip(glists, mlists, tU, tS):
        words += [len(g)] + list(g) + [len(m)] + list(m) + [repr(float(u)), repr(float(s))]
    p = str(d / "table.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_synthetic_table_rounds_batches_and_damaged_tables(harness):
    exe, d = harness
    table = synthetic_table(11, 20, 70)
    cls, pos_off, pos = table
    rng = np.random.default_rng(12)
    glists = [list(range(20)), [], rng.permutation(20)[:7].tolist(), [4]]
    mlists = [list(range(70)), [0, 1, 2], rng.permutation(70)[:65].tolist(), rng.permutation(70)[:2].tolist()]
    tU, tS = [0.5 * len(g) for g in glists], [0.25 * len(g) for g in glists]
    want = [plain_colocated(cls, pos_off, pos, g, m, 5000, 0.5) for g, m in zip(glists, mlists)]
    for budget, damaged in ((400, 150), (1 << 20, 0)):
        lines = run(exe, d, table, glists, mlists, tU, tS, 5000, 0.5, budget, damaged)
        assert lines[0] == "check rc=0"
        pairs = [tuple(int(x) for x in ln.split()) for ln in lines if len(ln.split()) == 4 and ln[0].isdigit()]
        assert pairs == [(q, i, j, n) for q, w in enumerate(want) for i, j, n in w] and len(pairs) > 20
        summary = [ln for ln in lines if ln.startswith("batches ")][0].split()
        assert (int(summary[1]) >= 3 and int(summary[3]) == 3) if budget == 400 else (int(summary[1]) == 1 and int(summary[3]) == 1)
        flags = [ln.split()[2] for ln in lines if ln.startswith("flags ")]
        assert flags == ["".join("%x" % v for v in plain_markers(cls, g, u, s)) for g, u, s in zip(glists, tU, tS)]
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged rc=0" in codes


def test_refused_calls(harness):
    exe, d = harness
    table = synthetic_table(13, 3, 4)
    cls, pos_off, pos = table
    ok = ([[0, 1]], [[0, 1, 2]], [1.0], [1.0])
    assert run(exe, d, table, *ok, 5000, 0.5, 64, 0)[0] == "check rc=0"
    assert run(exe, d, table, *ok, 4999.5, 0.5, 64, 0)[0] == "check rc=-1"
    big = pos.copy(); big[1] = 2**31
    assert run(exe, d, (cls, pos_off, big), *ok, 5000, 0.5, 64, 0)[0] == "check rc=-7"
    assert run(exe, d, table, [[0, 3]], [[0, 1]], [1.0], [1.0], 5000, 0.5, 64, 0)[0] == "check rc=-1"
    off = pos_off.copy(); off[2] = off[-1] + 1
    assert run(exe, d, (cls, off, pos), *ok, 5000, 0.5, 64, 0)[0] == "check rc=-1"
