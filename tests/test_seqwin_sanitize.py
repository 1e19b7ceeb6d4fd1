"""AddressSanitizer + UBSan over the host code of SequenceWindows: the window layout and the coding bases per window of the library
(nucstats_host.cpp: ckm_seq_windows_layout, ckm_seq_windows_coding over the GFF parsing of ckm_seq_genes_read), in a stand-alone program
(tests/native/seqwin_host_check.cpp).  Valid files must give the numpy mask's sums; damaged ones must be accepted or refused -- never
crash, never read or write outside a buffer.  No device needed."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import seqwin_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "seqwin_cases.json")))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("seqwin_sanitize")
    exe = str(d / "seqwin_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "seqwin_host_check.cpp"),
           os.path.join(CSRC, "nucstats_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, fasta, gff, w):
    out = subprocess.run([exe, fasta, gff, str(w)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return out.stdout.split("\n")


def test_valid_files_give_the_mask_sums(harness):
    exe, d = harness
    for case in GOLD["cases"]:
        if case["gff"] is None:
            continue
        fasta, gff = str(d / (case["name"] + ".fna")), str(d / (case["name"] + ".gff"))
        open(fasta, "w").write(case["fasta"])
        open(gff, "w").write(case["gff"])
        seqs, masks = ref.read_fasta(case["fasta"]), ref.coding_masks(case["gff"])
        for w in case["windows"]:
            lines = run(exe, fasta, gff, w)
            want = [int(np.sum(masks[k][x * w:(x + 1) * w])) if k in masks else 0 for k, s in seqs.items() for x in range(len(ref.windows(s, w)))]
            assert lines[0] == "rc=0 missing=0 windows=%d" % len(want) and [int(x) for x in lines[1].split()] == want
    lines = run(exe, fasta, str(d / "absent.gff"), 5)
    assert lines[0].startswith("rc=0 missing=1") and set(lines[1].split()) <= {"-1"}
    assert run(exe, fasta, gff, 0)[0].startswith("rc=-1 layout")


def test_damaged_gffs_are_accepted_or_refused(harness):
    exe, d = harness
    case = GOLD["cases"][0]
    fasta = str(d / "damaged.fna")
    open(fasta, "w").write(case["fasta"])
    r = random.Random(17)
    text = case["gff"].encode()
    rows = ["long\tx\tCDS\t0\t5\t.\t+\t0\tID=1\n", "long\tx\tCDS\t-7\t9999999999999\t.\t+\t0\tID=1\n", "long\tx\tCDS\t50\t10\t.\t+\t0\tID=1\n", "long\tx\tCDS\n",
            "long\tx\tCDS\t9223372036854775807\t9223372036854775807\t.\t+\t0\tID=1\n", "p29\tx\tCDS\tabc\t\t.\n", "\t\t\t\t\t\n"]
    codes = set()
    for k in range(24):
        body = bytearray(text)
        for _ in range(1 + k // 2):
            body[r.randrange(len(body))] = r.randrange(256)
        if k % 3 == 0:
            body += rows[(k // 3) % len(rows)].encode()
        if k % 8 == 7:
            body = body[:r.randrange(len(body))]
        gff = str(d / "damaged.gff")
        open(gff, "wb").write(bytes(body))
        for w in (1, 4, 7):
            codes.add(run(exe, fasta, gff, w)[0].split()[0])
    assert codes <= {"rc=0", "rc=-3", "rc=-2"} and "rc=0" in codes
