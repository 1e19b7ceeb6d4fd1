"""AddressSanitizer + UBSan over the host code of the all-pairs amino-acid identity: ckm_aai_check (aai_host.cpp) and the packing, the
batches, the pair decode and the per-chunk step of aai_dev.h, in a stand-alone program (tests/native/aai_host_check.cpp).  The golden
groups must give the reference's scores; damaged offset tables must be refused or walked -- never crash, never read or write outside a
buffer.  No device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from tests.test_aai_host import CASES, aai_plain, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("aai_sanitize")
    exe = str(d / "aai_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "aai_host_check.cpp"), os.path.join(CSRC, "aai_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, groups, budget, damaged):
    p = str(d / "groups.txt")
    open(p, "wb").write(b"".join(b"G %d\n" % len(g) + b"".join(b":" + r + b"\n" for r in g) for g in groups))
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def golden_groups(c):
    """The groups of a golden case in the sorted traversal: (rows, the reference's scores)."""
    out = []
    for rel in sorted(c["files"]):
        if not rel.endswith(".masked.faa"):
            continue
        lines = c["files"][rel].split("\n")
        rows = [lines[k + 1] for k, ln in enumerate(lines) if ln.startswith(">")]              # one line per sequence in these cases, empty ones too
        _q, _a, binId, name = rel.split("/")
        out.append(([r.encode() for r in rows], binId, name[:name.find(".")]))
    return out


def test_golden_groups_give_the_references_scores(harness):
    exe, d = harness
    for name in ("basic", "column_zero", "no_report"):
        c = CASES[name]
        groups = golden_groups(c)
        lines = run(exe, d, [g for g, _b, _m in groups], 64, 0)
        assert lines[0] == "check rc=0" and int([x for x in lines if x.startswith("batches ")][0].split()[1]) >= 2
        got = {}
        for ln in lines[1:]:
            f = ln.split()
            if len(f) == 6:
                _rows, binId, marker = groups[int(f[0])]
                got.setdefault(binId, {}).setdefault(marker, []).append(float(f[5]))
        assert got == c["raw"]


def test_synthetic_counts_and_damaged_tables(harness):
    exe, d = harness
    groups, want = synthetic()
    groups, want = groups[:-4], want[:len(want) - 44850]                 # without the 300 copies: the host executor's test covers them
    lines = run(exe, d, groups, 1 << 14, 300)
    assert lines[0] == "check rc=0"
    pairs = [ln.split() for ln in lines if len(ln.split()) == 6]
    assert [(int(f[3]), int(f[4]), float(f[5])) for f in pairs] == [tuple(w) for w in want]
    codes = [ln for ln in lines if ln.startswith("damaged rc=")]
    assert len(codes) == 300 and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"} and "damaged rc=-1" in codes
    lines = run(exe, d, [[b"AC", b"A"], [b"A" * 4097, b"C" * 4097]], 64, 0)
    assert lines[0] == "check rc=-1"
    assert run(exe, d, [[b"A" * 4097, b"C" * 4097]], 64, 0)[0] == "check rc=-7"
    assert aai_plain(b"A-", b"AC") == (0, 1, 1.0)
