"""AddressSanitizer + UBSan over the host code of the placement: ckm_place_check (place_host.cpp) and the tests, the level schedule, the
chunk cuts and the arithmetic of place_dev.h walked by its host executor, in a stand-alone program
(tests/native/placement_host_check.cpp).  The seeded case must give the executor's own results under budgets that cut the sites into
several chunks; damaged calls must be refused or walked -- never crash, never read or write outside a buffer.  No device needed, nothing
is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd.pplacer import PplacerRunner
from tests.emu import placement as emu
from tests.emu import placement_oracle as orc
from tests.test_placement_host import small_tables, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("placement_sanitize")
    exe = str(d / "placement_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "placement_host_check.cpp"),
           os.path.join(CSRC, "place_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, t, budget, damaged):
    words = [t.nnodes, t.child.shape[0], t.nsites, t.nrows, t.nqueries, t.nrates, t.nfrac, t.npend, t.max_pitches]
    words += t.child_off.tolist() + t.child.tolist() + [float(x).hex() for x in t.length] + t.row_off.tolist() + t.rows.tolist() + t.q_off.tolist() + t.queries.tolist()
    for a in (t.weights, t.U, t.Uinv, t.pi, t.exp_len, t.exp_half, t.exp_dist, t.exp_pend):
        words += [float(x).hex() for x in a.reshape(-1)]
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def test_seeded_case_budgets_and_damaged_calls(harness):
    exe, d = harness
    rng = np.random.default_rng(8)
    ref, aln, _ = synthetic(9, orc.random_tree(rng, 6, 0.0, 0.5, root_degree=3), 150)
    t = PplacerRunner(1)._tables(ref, {"a": aln["t1"], "b": aln["t4"][:70] + "-" * 80, "c": "x" * 150}, (0.05, 0.5), (0.25, 0.75), 0.1, 4)
    for budget, damaged, chunks in ((1, 120, 3), (1 << 30, 0, 1)):
        want = emu.place_run(None, t, budget)
        lines = run(exe, d, t, budget, damaged)
        assert lines[0] == "check rc=0"
        rows = [ln.split() for ln in lines if len(ln.split()) == 9]
        assert len(rows) == 3 * 4 and int([ln for ln in lines if ln.startswith("chunks ")][0].split()[1]) == chunks == want["nchunks"]
        for r in rows:
            q, k = int(r[0]), int(r[1])
            assert int(r[2]) == want["top_edge"][q, k] and float.fromhex(r[3]) == want["scan_m"][q, k] and int(r[4]) == want["scan_e"][q, k]
            assert float.fromhex(r[5]) == want["ref_m"][q, k] and int(r[6]) == want["ref_e"][q, k] and (int(r[7]), int(r[8])) == (want["ref_f"][q, k], want["ref_g"][q, k])
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged rc=0" in codes


def test_refused_calls(harness):
    exe, d = harness
    assert run(exe, d, small_tables(), 64, 0)[0] == "check rc=0"
    assert run(exe, d, small_tables(length=[0.1, -0.2, 0.3, 0.0]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(row_off=[0, 4, 9, 12]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(child=[0, 1, 1]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(child_off=[0, 0, 3, 2, 3]), 64, 0)[0] == "check rc=-1"
    assert run(exe, d, small_tables(R=9), 64, 0)[0] == "check rc=-7"
