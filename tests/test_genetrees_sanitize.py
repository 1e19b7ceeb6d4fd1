"""AddressSanitizer + UBSan over the host code of the gene-tree tests: ckm_genetree_check and the host executor ckm_genetree_host
(genetree_host.cpp) with the checks, the walks, the quotients and the round cuts of genetree_dev.h, in a stand-alone program
(tests/native/genetrees_host_check.cpp).  The seeded forest must give the emulator's outputs under budgets that cut the call into one
round per tree, a few and one; damaged calls -- ranges outside the tree, a parent behind its child, a class index beyond the class count,
a pair that names a leaf beyond the tree -- must be refused or run: never crash, never read or write outside a buffer.  No device needed,
nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd import geneTrees
from tests import genetrees_synth as synth
from tests.emu import genetrees as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("genetrees_sanitize")
    exe = str(d / "genetrees_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "genetrees_host_check.cpp"),
           os.path.join(CSRC, "genetree_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, t, budget, damaged):
    words = [t.ntrees]
    for f in ("node_off", "leaf_off", "group_off", "class_off", "gpair_off", "first", "last", "parent", "internal"):
        words += getattr(t, f).tolist()
    words += [float(x).hex() for x in t.length.tolist()]
    for f in ("leaf_genome", "leaf_species", "leaf_class", "class_total", "pair_a", "pair_b"):
        words += getattr(t, f).tolist()
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def forest_tables():
    md = synth.metadata(17)
    specs = [("r0", "random", 27, 17, ((1, 3), (4, 2)), 0.3), ("r1", "chain", 14, 6, ((0, 4),), 0.4), ("r2", "star", 9, 4, (), 0.5), ("r3", "random", 2, 17, (), 0.0),
             ("r4", "caterpillar", 22, 8, ((2, 2),), 0.2), ("r5", "balanced", 16, 5, (), 0.1)]
    return geneTrees.forestTables([geneTrees.packTree(n, t, md, geneTrees.genomeIdOfGene) for n, t in synth.forest(61, specs)])


def test_seeded_forest_rounds_and_damaged_calls(harness):
    exe, d = harness
    t = forest_tables()
    want = emu.genetree_run(None, t)
    sizes = [emu.tree_bytes(t, k) for k in range(t.ntrees)]
    for budget, damaged in ((1, 400), (2 * max(sizes), 0), (1 << 30, 0)):
        lines = run(exe, d, t, budget, damaged)
        assert lines[0] == "check rc=0"
        assert [float.fromhex(ln.split()[2]) for ln in lines if ln.startswith("c ")] == want["consistency"].tolist()
        assert [int(ln.split()[2]) for ln in lines if ln.startswith("p ")] == want["pair_flag"].tolist()
        assert [[int(x) for x in ln.split()[2:]] for ln in lines if ln.startswith("g ")] == np.stack([want["group_node"], want["group_mixed"]], axis=1).tolist()
        assert int([ln for ln in lines if ln.startswith("rounds ")][0].split()[1]) == emu.rounds(t, budget)
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=0" in codes
    assert emu.rounds(t, 1) == t.ntrees and 1 < emu.rounds(t, 2 * max(sizes)) < t.ntrees and emu.rounds(t, 1 << 30) == 1


def test_refused_calls(harness):
    exe, d = harness
    md = synth.metadata(6)
    p = geneTrees.packTree("t", "((G1|a:0.1,G1|b:0.2):0.1,(G2|a:0.3,G3|a:0.1):0.2,G1|c:0.0);", md)

    def first_line(change):
        t = geneTrees.forestTables([p])
        change(t)
        return run(exe, d, t, 64, 0)[0]

    assert first_line(lambda t: None) == "check rc=0"
    assert first_line(lambda t: t.last.__setitem__(1, 9)) == "check rc=-1"
    assert first_line(lambda t: t.first.__setitem__(3, 7)) == "check rc=-1"
    assert first_line(lambda t: t.parent.__setitem__(2, 5)) == "check rc=-1"
    assert first_line(lambda t: t.leaf_class.__setitem__(3, 4)) == "check rc=-1"
    assert first_line(lambda t: t.pair_b.__setitem__(1, 5)) == "check rc=-1"
    assert first_line(lambda t: t.length.__setitem__(1, float("inf"))) == "check rc=-1"
    many = synth.metadata((1 << 14) + 1, one_class=True)
    big = geneTrees.packTree("big", "(" + ",".join("G%d|x:0.1" % k for k in range((1 << 14) + 1)) + ");", many)
    assert run(exe, d, geneTrees.forestTables([big]), 64, 0)[0] == "check rc=-7"
