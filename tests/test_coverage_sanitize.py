"""AddressSanitizer + UBSan over the host side of `checkm coverage`: the BGZF / BAM reader of the library (bam_host.cpp) and the host
executor of the device pass (coverage_dev.h through tests/emu/coverage_emu.cpp).  Damaged files must be accepted or refused -- never
crash, never read outside a buffer; the damage inside a BGZF block is caught by its CRC, so the records are also damaged before they
are compressed.  No device needed."""
import json
import os
import random
import shutil
import subprocess

import pytest

from synthdata import bam as sbam
from tests import coverage_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("cov_sanitize")
    exe = str(d / "coverage_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-ffp-contract=off",
           "-I", CSRC, os.path.join(ROOT, "tests", "native", "coverage_host_check.cpp"), os.path.join(ROOT, "tests", "emu", "coverage_emu.cpp"),
           os.path.join(CSRC, "bam_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def _run(exe, path, work, rounds, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, path, str(work), str(rounds), str(seed)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-4000:])
    return json.loads(out.stdout.strip().split("\n")[-1])


def test_reader_survives_damaged_files(harness):
    exe, d = harness
    refs, recs = cr.synthetic(1500, 20, seed=2)
    path = str(d / "valid.bam")
    sbam.write_bam(path, refs, recs, block_bytes=3000, empty_every=5)
    got = _run(exe, path, d, 300, 21)
    assert got["records"] == 1500 and got["rejected"] >= 150


def test_record_logic_survives_damaged_records(harness):
    """Damage under the CRC: bytes of the inflated records are changed before compression, so the walk over the fixed part, the CIGAR and
    the auxiliary fields sees lengths, counts and types that lie."""
    exe, d = harness
    r = random.Random(4)
    refs, recs = cr.synthetic(400, 5, seed=9)
    head = sbam.header_bytes(refs)
    accepted = rejected = 0
    for k in range(12):
        body = bytearray(b"".join(sbam.record_bytes(x) for x in recs))
        for _ in range(1 + k):
            body[r.randrange(len(body))] = r.randrange(256)
        path = str(d / "lying.bam")
        with open(path, "wb") as f:
            f.write(sbam.bgzf(head + bytes(body), block_bytes=5000))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, path, str(d), "0", "1"], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode in (0, 1) and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
        accepted += out.returncode == 0
        rejected += out.returncode == 1
    assert accepted + rejected == 12
