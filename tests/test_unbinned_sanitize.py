"""AddressSanitizer + UBSan over the host code of Unbinned: the id reader (nucstats_host.cpp: ckm_fasta_ids_read), the selection and the
writer (unbinned_host.cpp) and the tile geometry of unbinned_dev.h, in a stand-alone program (tests/native/unbinned_host_check.cpp).
The golden inputs must give the reference's files; damaged FASTA files must be accepted or refused -- never crash, never read or write
outside a buffer.  No device needed, nothing is loaded into python."""
import os
import random
import shutil
import subprocess

import pytest

from tests.test_unbinned_host import GOLD, write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("unbinned_sanitize")
    exe = str(d / "unbinned_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "unbinned_host_check.cpp"),
           os.path.join(CSRC, "nucstats_host.cpp"), os.path.join(CSRC, "unbinned_host.cpp"), "-lz", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, min_len, asm, bins):
    seqOut, statsOut = str(d / "out.fna"), str(d / "out.tsv")
    for p in (seqOut, statsOut):
        if os.path.exists(p):
            os.remove(p)
    out = subprocess.run([exe, str(min_len), seqOut, statsOut, asm] + bins, capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode("utf-8", errors="replace").split("\n"), seqOut, statsOut


def test_golden_inputs_give_the_references_files(harness):
    exe, top = harness
    for c in GOLD["cases"]:
        if c["assembly"] is None:
            continue
        d = top / c["name"]
        d.mkdir()
        bins, asm = write_inputs(d, c)
        lines, seqOut, statsOut = run(exe, d, c["minSeqLen"], asm, bins)
        assert lines[0] == "ids rc=0" and "assembly rc=0" in lines
        w = [x for x in lines if x.startswith("write rc=")][0]
        assert w.startswith("write rc=0 zero=") and (int(w.split("=")[2]) >= 0) == (c["error"] is not None and c["out_stats"].count("\n") - 1 < c["out_seq"].count(">"))
        assert open(seqOut, "rb").read().decode("utf-8") == c["out_seq"] and open(statsOut, "rb").read().decode("utf-8") == c["out_stats"]


def test_damaged_files_are_accepted_or_refused(harness):
    exe, d = harness
    c = [x for x in GOLD["cases"] if x["name"] == "utf8"][0]
    base = c["assembly"].encode("utf-8") + b">long one\n" + b"ACGTNacgtu" * 40 + b"\n"
    r = random.Random(19)
    fixed = [b">", b">\n", b">>>>\n>\n", b"> \nACGT\n", b">\t\n", b"ACGT\n>late\nAC\n", b"", b"\n\n\n", b">a", b">a\n\xff\xfe\n", b">a\n" + b"\xc3", b">\xe2\x82\n", b">a\r", b">a\rA",
             b">dup\nAC\n>dup\n>dup\nA"]
    codes = set()
    for k in range(40):
        if k < len(fixed):
            body = fixed[k]
        else:
            body = bytearray(base)
            for _ in range(1 + k // 4):
                body[r.randrange(len(body))] = r.randrange(256)
            if k % 5 == 4:
                body = body[:r.randrange(len(body))]
            body = bytes(body)
        p = str(d / "damaged.fna")
        open(p, "wb").write(body)
        lines, _s, _t = run(exe, d, k % 3 * 5, p, [p, p])       # as the assembly and as two bins: every id is binned
        codes.add(lines[0])
        if lines[0] == "ids rc=0":
            assert "assembly rc=0" in lines and [x for x in lines if x.startswith("write rc=0 zero=-1")]
        good = str(d / "good.fna")
        open(good, "wb").write(base)
        lines, _s, _t = run(exe, d, 0, p, [good])               # as the assembly against an intact bin
        codes.add([x for x in lines if x.startswith("assembly rc=")][0])
    assert codes <= {"ids rc=0", "ids rc=-3", "assembly rc=0", "assembly rc=-3"} and len(codes) == 4
