"""AddressSanitizer + UBSan over the host code of ReferenceDistributions: the scaffold join and the argument checks (refdist_dev.h,
ckm_refdist_check) and the coding bases of windows anywhere in a sequence (nucstats_host.cpp: ckm_refdist_coding over the GFF parsing of
ckm_seq_genes_read), in a stand-alone program (tests/native/refdist_host_check.cpp).  Valid files must give the scaffold and the numpy
mask's sums; damaged ones must be accepted or refused -- never crash, never read or write outside a buffer.  No device needed."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests import refdist_reference as ref
from tests.seqwin_reference import coding_masks, read_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "refdist_cases.json")))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("refdist_sanitize")
    exe = str(d / "refdist_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "refdist_host_check.cpp"),
           os.path.join(CSRC, "nucstats_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, fasta, gff, seqId, sep):
    out = subprocess.run([exe, fasta, gff, seqId, str(sep)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return out.stdout.split("\n")


def windows(L):
    return [(7 * k, 1 + 13 * (k % 9)) for k in range(-(-(L + 20) // 7))]


def test_valid_files_give_the_scaffold_and_the_mask_sums(harness):
    exe, d = harness
    for case in GOLD["cases"]:
        fasta, gff = str(d / (case["name"] + ".fna")), str(d / (case["name"] + ".gff"))
        open(fasta, "w").write(case["fasta"])
        open(gff, "w").write(case["gff"] or "##gff-version  3\n")
        seqs = read_fasta(case["fasta"])
        mask = coding_masks(case["gff"] or "").get(case["name"])
        for stat, sep in (("gc", 0), ("td", 4), ("cd", 10)):
            raw = ("N" * sep).join(seqs.values())
            L = len(raw)
            lines = run(exe, fasta, gff, case["name"], sep)
            assert lines[0] == "scaffold=%d buffer=%d" % (L, (L + 15) // 16 * 16 + 64) and lines[1] == raw and lines[1].upper() == ref.scaffold(seqs, stat).upper()
            assert lines[2] == ("check=0 0 -1 -1 -1 -1 -1 -1 0 -1" if L else "check=-1 -1 -1 -1 -1 -1 -1 -1 0 -1")
            want = [int(np.sum(mask[s:s + w])) if mask is not None else 0 for s, w in windows(L)]
            assert lines[3] == "rc=0 total=%d windows=%d" % (int(np.sum(mask)) if mask is not None else 0, len(want)) and [int(x) for x in lines[4].split()] == want
    assert run(exe, fasta, str(d / "absent.gff"), "x", 10)[3].startswith("rc=-2")


def test_damaged_gffs_are_accepted_or_refused(harness):
    exe, d = harness
    case = [c for c in GOLD["cases"] if c["name"] == "genes"][0]
    fasta = str(d / "damaged.fna")
    open(fasta, "w").write(case["fasta"])
    r = random.Random(18)
    text = case["gff"].encode()
    rows = ["genes\tx\tCDS\t0\t5\t.\t+\t0\tID=1\n", "genes\tx\tCDS\t-7\t9999999999999\t.\t+\t0\tID=1\n", "genes\tx\tCDS\t50\t10\t.\t+\t0\tID=1\n", "genes\tx\tCDS\n",
            "genes\tx\tCDS\t9223372036854775807\t9223372036854775807\t.\t+\t0\tID=1\n", "genes\tx\tCDS\tabc\t\t.\n", "\t\t\t\t\t\n"]
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
        codes.add(run(exe, fasta, gff, "genes", 10)[3].split()[0])
    assert codes <= {"rc=0", "rc=-3", "rc=-2"} and "rc=0" in codes
