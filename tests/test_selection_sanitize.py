"""AddressSanitizer + UBSan over the host code of the marker-set selection: ckm_select_check (select_host.cpp) and the generator, the draw,
the packing and the round cuts of select_dev.h, in a stand-alone program (tests/native/selection_host_check.cpp).  The seeded synthetic
case must give the plain-Python path's results under budgets that cut the call into many rounds; damaged calls must be refused or
walked -- never crash, never read or write outside a buffer.  No device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from checkm_amd.markerSetBuilder import MarkerSetBuilder
from tests.test_selection_host import builder_case, small_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("selection_sanitize")
    exe = str(d / "selection_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "selection_host_check.cpp"),
           os.path.join(CSRC, "select_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, t, budget, damaged):
    words = [t.ngenomes, t.nmarkers, t.nsets, t.nreplicates, t.key.shape[0], t.cs_off.shape[0] - 1, t.cs_marker.shape[0], t.contig_len, t.seed]
    words += [float(x).hex() for x in (t.comp_lo, t.comp_hi, t.cont_lo, t.cont_hi)]
    for a in (t.genome_len, t.key_off, t.key, t.ms_off, t.cs_off, t.cs_marker):
        words += a.tolist()
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_synthetic_case_rounds_and_damaged_calls(harness):
    exe, d = harness
    b = MarkerSetBuilder(None)
    sets, positions, sizes = builder_case(5)
    R, args = 6, (1000, (0.5, 1.0), (0.0, 0.7), 77)
    true, want, mults = b._sampled_checks_host(sets, positions, sizes, R, *args)
    tables = b._select_tables(sets, positions, sizes, R, *args)
    draws = len(sizes) * R
    for budget, damaged in ((1, 200), (1000, 0), (1 << 30, 0)):
        lines = run(exe, d, tables, budget, damaged)
        assert lines[0] == "check rc=0"
        heads = [ln.split() for ln in lines if len(ln.split()) == 5 and not ln.startswith(("check", "damaged", "error"))]
        assert [(int(h[0]), int(h[1])) for h in heads] == [(g, r) for g in range(len(sizes)) for r in range(R)]
        assert [[float.fromhex(h[2]), float.fromhex(h[3])] for h in heads] == true.reshape(-1, 2).tolist()
        assert [int(h[4]) for h in heads] == [int(m[r].sum()) for m in mults for r in range(R)]
        rows = [ln.split() for ln in lines if len(ln.split()) == 7]
        assert [(int(r[0]), int(r[1]), int(r[2])) for r in rows] == [(g, r, s) for g in range(len(sizes)) for r in range(R) for s in range(len(sets))]
        assert [[float.fromhex(v) for v in r[3:]] for r in rows] == want.reshape(-1, 4).tolist()
        rounds = int([ln for ln in lines if ln.startswith("rounds ")][0].split()[1])
        assert rounds == draws if budget == 1 else 1 < rounds < draws if budget == 1000 else rounds == 1
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged rc=0" in codes


def test_refused_calls(harness):
    exe, d = harness
    assert run(exe, d, small_tables(), 64, 0)[0] == "check rc=0"
    assert run(exe, d, small_tables(genome_len=[16385 * 1000, 3000]), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(genome_len=[10500, 999]), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(comp=(0.5, 1.5)), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(cont=(0.3, 0.2)), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(keys=[[[10, 2**31], [], [9000]], [[5], [2999], []]]), 64, 0)[0] == "check rc=-7"
    assert run(exe, d, small_tables(key_off=[0, 2, 1, 3, 4, 6, 6]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(cs_off=[0, 2, 2, 6]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(ms_off=[0, 2, 2]), 64, 0)[0] == "check rc=-1"
