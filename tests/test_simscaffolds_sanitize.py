"""AddressSanitizer + UBSan over the host code of the scaffold simulation: ckm_simscaf_check (simscaf_host.cpp) and the packing, the round
cuts and the per-copy step of simscaf_dev.h, in a stand-alone program (tests/native/simscaf_host_check.cpp).  The seeded synthetic case
must give the plain loop's results under budgets that cut the call into many rounds; damaged calls must be refused or walked -- never
crash, never read or write outside a buffer.  No device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from tests.test_simscaffolds_host import small_tables, synthetic_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("simscaffolds_sanitize")
    exe = str(d / "simscaf_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "simscaf_host_check.cpp"),
           os.path.join(CSRC, "simscaf_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, t, budget, damaged):
    words = [t.ngenomes, t.nmarkers, t.nsets, t.nreplicates, t.sc.shape[0], t.cs_off.shape[0] - 1, t.cs_marker.shape[0], t.bits.shape[0]]
    for a in (t.nscaf, t.sc_off, t.sc, t.ms_off, t.cs_off, t.cs_marker, t.test, t.cont, t.bit_off, t.bits):
        words += a.tolist()
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_synthetic_case_rounds_and_damaged_calls(harness):
    exe, d = harness
    b, sets, test, draws = synthetic_case(5)
    want = b._scaffold_checks_host(sets, test, draws)
    tables = b._scaffold_tables(sets, test, draws)
    for budget, damaged in ((1, 200), (700, 0), (1 << 30, 0)):
        lines = run(exe, d, tables, budget, damaged)
        assert lines[0] == "check rc=0"
        rows = [ln.split() for ln in lines if len(ln.split()) == 6]
        assert [(int(r[0]), int(r[1])) for r in rows] == [(x, y) for x in range(len(draws)) for y in range(len(sets))]
        assert [[float.fromhex(v) for v in r[2:]] for r in rows] == want.reshape(-1, 4).tolist()
        rounds = int([ln for ln in lines if ln.startswith("rounds ")][0].split()[1])
        assert rounds == len(draws) if budget == 1 else 1 < rounds < len(draws) if budget == 700 else rounds == 1
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged rc=0" in codes


def test_refused_calls(harness):
    exe, d = harness
    assert run(exe, d, small_tables(), 64, 0)[0] == "check rc=0"
    assert run(exe, d, small_tables(nscaf=[33, 2**30 + 1]), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(sc=[33, 0, 0, 2, 1, 1]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(cont=[2, 0xffffffff, 0]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(bit_off=[0, 2, 4, 8]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(bits=[1, 2, 5, 7, 0xffffffff, 1, 0, 0]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(cs_off=[0, 2, 2, 5]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(ms_off=[0, 3, 3]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(bit_off=[0, 3, 4, 9]), 64, 0)[0] == "check rc=-1"
