"""The search under the stream plans of different hardware-queue budgets (csrc/stream_plan.h): the rows of the domain tables and the
lanes handed to the host-driven cascade do not depend on how many streams the pool holds, nor on two contexts sharing them.  Every case
is a fresh child process -- the setting has to be in place before HIP starts."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the mixed world of test_gpu_cascade.py as a dozen smaller bins: every model-length class of the mixed profiles, two sequence parts
# (CKM_SPLIT_MIN_PAIRS=1), a tandem repeat in every other bin (multi-domain regions -> the ensemble stream)
CODE = r'''
import sys, json, os, tempfile, threading
sys.path.insert(0, %r)
import numpy as np
from checkm_amd import _lib
from synthdata import synth
from tests import common
profs = common.mixed_profiles(); path = common.hmm_file("mixed", profs)
rng = np.random.default_rng(5)
NB = 12
bins = [synth.make_bin(profs, 8800 + b, n_orfs=130, dup_frac=0.4) for b in range(NB)]
for b in range(0, NB, 2):
    p = profs[3 + b %% 6]
    a, c = p.M * 3 // 4, p.M // 3
    t = np.concatenate([synth.random_residues(rng, 9), synth.sample_domain(rng, p, 1, a), synth.sample_domain(rng, p, c, p.M), synth.random_residues(rng, 8)])
    bins[b].append(("tandem%%d_1" %% b, "", synth.to_text(t) + "*"))
tmp = tempfile.mkdtemp()

def one(tag, nrep):
    ctx = _lib.Context(0); prof = _lib.Profiles(ctx, path); seqs = _lib.Seqs(ctx, bins)
    runs = []
    for rep in range(nrep):
        hits = _lib.search(ctx, prof, seqs)
        st = ctx.stats()
        text = []
        for b in range(NB):
            f = os.path.join(tmp, "%%s_%%d_%%d.domtblout" %% (tag, rep, b))
            hits.write_domtblout(prof, seqs, b, f)
            text.append("".join(ln for ln in open(f, newline="") if not ln.startswith("#")))       # the rows, byte for byte
        runs.append({"domtblout": text, "fallback": int(st.cascade_fallback_lanes), "regions_multi": int(st.regions_multi), "pairs_ssv": int(st.pairs_ssv)})
        hits.close()
    return runs

nthreads = int(os.environ.get("CKM_TEST_THREADS", "1"))
out = [None] * nthreads
def work(k): out[k] = one("t%%d" %% k, 2 if nthreads > 1 else 1)
th = [threading.Thread(target=work, args=(k,)) for k in range(nthreads)]
for t in th: t.start()
for t in th: t.join()
print(json.dumps({"runs": [r for o in out for r in o]}))
''' % ROOT

CHILD_TIMEOUT = 120          # seconds: a child takes a few


def _run(unset=(), **extra):
    env = dict(os.environ, CKM_WORKERS="1", CKM_SPLIT_MIN_PAIRS="1", **extra)
    for k in unset:
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", CODE], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0, (extra, out.stderr[-3000:])
    return json.loads(out.stdout.strip().split("\n")[-1])["runs"]


@pytest.fixture(scope="module")
def default_run():
    """the environment as inherited"""
    r = _run(unset=("CKM_HW_QUEUES", "CKM_STREAM_LAYOUT"))[0]
    assert r["fallback"] == 0
    assert r["regions_multi"] >= 2                                        # the ensemble stream is used
    assert sum(len([ln for ln in t.splitlines() if ln and not ln.startswith("#")]) for t in r["domtblout"]) > 100
    return r


@pytest.mark.parametrize("setting", [("GPU_MAX_HW_QUEUES", "4"), ("GPU_MAX_HW_QUEUES", "6"), ("GPU_MAX_HW_QUEUES", "16"),
                                     ("CKM_HW_QUEUES", "4"), ("CKM_HW_QUEUES", "6"), ("CKM_HW_QUEUES", "16")])
def test_rows_do_not_depend_on_the_queue_budget(default_run, setting):
    """GPU_MAX_HW_QUEUES: the runtime's queues and the plan follow the value; CKM_HW_QUEUES: the plan alone, on the queues as inherited"""
    r = _run(unset=("CKM_HW_QUEUES", "CKM_STREAM_LAYOUT"), **{setting[0]: setting[1]})[0]
    assert r["pairs_ssv"] == default_run["pairs_ssv"]
    assert r["fallback"] == default_run["fallback"]
    assert r["domtblout"] == default_run["domtblout"]


@pytest.mark.parametrize("layout", [None, "2,2,0,0", "4,0,0,0"])
def test_two_contexts_in_flight_at_four_queues(default_run, layout):
    """two threads, a context each, two searches each on one device, as find() keeps them: at four queues the contexts share every handle
    of the pool.  layout: the plan's own (1 SSV + 3 chain handles); two SSV handles; the chains on the four SSV handles themselves."""
    extra = {"CKM_STREAM_LAYOUT": layout} if layout else {}
    runs = _run(unset=("CKM_HW_QUEUES",) + (() if layout else ("CKM_STREAM_LAYOUT",)), GPU_MAX_HW_QUEUES="4", CKM_TEST_THREADS="2", **extra)
    assert len(runs) == 4
    for r in runs:
        assert r["fallback"] == default_run["fallback"]
        assert r["domtblout"] == default_run["domtblout"]
