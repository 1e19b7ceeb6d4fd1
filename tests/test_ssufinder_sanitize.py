"""AddressSanitizer + UBSan over the host code of the nucleotide model scan: ckm_nhmm_check (nhmm_host.cpp) and the check, the tile cuts,
the recurrence, the compaction and the hit rule of nhmm_dev.h walked by its host executor, in a stand-alone program
(tests/native/ssufinder_host_check.cpp).  The seeded case must give the executor's own rows and hits under two budgets; damaged calls
must be refused or walked -- never crash, never read or write outside a buffer.  No device needed, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.hmmerModelParser import read_nuc_models
from tests import ssufinder_synth as syn
from tests.emu import ssufinder as emu
from tests.test_ssufinder_host import HIT_F, ROW_F, read_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("ssufinder_sanitize")
    exe = str(d / "ssufinder_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "ssufinder_host_check.cpp"),
           os.path.join(CSRC, "nhmm_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(exe, d, tables, records, budget, damaged):
    words = [tables.nmodels, tables.stride, tables.overlap, tables.strands, len(records)] + tables.M.tolist() + tables.min_score.tolist() + tables.emis.tolist() + tables.trans.tolist()
    words += [len(s) for _, s in records] + [b for _, s in records for b in s.encode("latin-1")]
    p = str(d / "call.txt")
    open(p, "w").write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, p, str(budget), str(damaged)], capture_output=True, timeout=300, env=dict(os.environ, **ENV))
    err = out.stderr.decode(errors="replace")
    assert out.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return out.stdout.decode().split("\n")


def seeded(tmp_path):
    models = []
    cons = []
    for k, M in enumerate((12, 70)):
        p = str(tmp_path / ("m%d.hmm" % M))
        cons.append(syn.write_model(p, "m%d" % M, M, 50 + k))
        m = read_nuc_models(p)[0]
        models.append((m.emis, m.trans))
    rng = np.random.default_rng(5)
    records = [("a", syn.planted_contig(rng, 260, [(30, cons[0], False), (100, cons[1], True)])[0]), ("b", ""), ("c", "acgNNu"), ("d", syn.random_dna(rng, 64))]
    return _lib.NhmmTables(models, [5000, -(1 << 20)], 64, 32, 3), records


def test_seeded_case_budgets_and_damaged_calls(harness, tmp_path):
    exe, d = harness
    tables, records = seeded(tmp_path)
    seqs = read_seqs(tmp_path, records)
    for budget, damaged in ((1, 150), (1 << 30, 0)):
        want = emu.nhmm_run(None, tables, seqs, budget)
        lines = run(exe, d, tables, records, budget, damaged)
        assert lines[0] == "check rc=0" and "walk rc=0" in lines
        rows = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("r ")]
        hits = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("h ")]
        assert rows == list(zip(*[want[f].tolist() for f in ROW_F])) and hits == list(zip(*[want[f].tolist() for f in HIT_F])) and len(hits) >= 2
        assert int([ln for ln in lines if ln.startswith("batches ")][0].split()[1]) == want["batches"]
        codes = [ln for ln in lines if ln.startswith("damaged rc=")]
        walks = [ln for ln in lines if ln.startswith("damaged walk rc=")]
        assert len(codes) == damaged and set(codes) <= {"damaged rc=0", "damaged rc=-1", "damaged rc=-7"} and set(walks) <= {"damaged walk rc=0", "damaged walk rc=1"}
        if damaged:
            assert "damaged rc=-1" in codes and "damaged rc=-7" in codes and "damaged walk rc=0" in walks and "damaged walk rc=1" in walks
    seqs.close()


def test_refused_calls(harness, tmp_path):
    exe, d = harness
    tables, records = seeded(tmp_path)
    assert run(exe, d, tables, records, 64, 0)[0] == "check rc=0"
    for field, value, rc in (("stride", 0, -1), ("strands", 7, -1), ("overlap", 1 << 17, -7)):
        t, _ = seeded(tmp_path)
        setattr(t, field, value)
        assert run(exe, d, t, records, 64, 0)[0] == "check rc=%d" % rc
    t, _ = seeded(tmp_path)
    t.min_score[0] = -(1 << 20) - 1
    assert run(exe, d, t, records, 64, 0)[0] == "check rc=-7"
    t, _ = seeded(tmp_path)
    t.trans[5] = 1
    assert run(exe, d, t, records, 64, 0)[0] == "check rc=-7"
    assert run(exe, d, tables, records + [("e", "AC\xe9T")], 64, 0)[:2] == ["check rc=0", "walk rc=1"]
