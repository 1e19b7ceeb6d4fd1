"""AddressSanitizer + UBSan over the host side of CoverageWindows: the BGZF / BAM reader of the library (bam_host.cpp) and the host
executor of the device pass (covwin_dev.h through tests/emu/covwin_emu.cpp: the chain, the reference span of the CIGAR, the scatter
into the window arrays and the scan), in a stand-alone program (tests/native/covwin_host_check.cpp).  Damaged files must be accepted
or refused -- never crash, never read or write outside a buffer; the damage inside a BGZF block is caught by its CRC, so the records
are also damaged before they are compressed: positions, CIGAR lengths and reference lengths that lie.  No device needed."""
import json
import os
import random
import shutil
import subprocess

import pytest

from synthdata import bam as sbam
from tests import covwin_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("covwin_sanitize")
    exe = str(d / "covwin_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-ffp-contract=off",
           "-I", CSRC, os.path.join(ROOT, "tests", "native", "covwin_host_check.cpp"), os.path.join(ROOT, "tests", "emu", "covwin_emu.cpp"),
           os.path.join(CSRC, "bam_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def test_reader_and_scatter_survive_damaged_files(harness):
    exe, d = harness
    refs, recs = wr.synthetic(1500, 20, seed=2)
    path = sbam.write_bam(str(d / "valid.bam"), refs, recs, block_bytes=3000, empty_every=5)
    out = subprocess.run([exe, path, str(d), "300", "21"], capture_output=True, text=True, timeout=600, env=dict(os.environ, **ENV))
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-4000:])
    got = json.loads(out.stdout.strip().split("\n")[-1])
    assert got["records"] == 1500 and got["rejected"] >= 150 and got["slots"] > sum(n for _n, n in refs)


def test_record_logic_survives_damaged_records(harness):
    """Damage under the CRC: bytes of the header and of the inflated records are changed before compression, so the chain, the CIGAR walk,
    the scatter and the layout see positions, lengths, counts and types that lie."""
    exe, d = harness
    r = random.Random(4)
    refs, recs = wr.synthetic(400, 5, seed=9)
    head = sbam.header_bytes(refs)
    accepted = rejected = 0
    for k in range(12):
        body = bytearray(head + b"".join(sbam.record_bytes(x) for x in recs))
        for _ in range(1 + k):
            body[r.randrange(len(head) - 30 if k % 4 == 3 else 0, len(body))] = r.randrange(256)
        path = str(d / "lying.bam")
        with open(path, "wb") as f:
            f.write(sbam.bgzf(bytes(body), block_bytes=5000))
        out = subprocess.run([exe, path, str(d), "0", "1"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
        assert out.returncode in (0, 1) and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
        accepted += out.returncode == 0
        rejected += out.returncode == 1
    assert accepted + rejected == 12
