"""The float stages of the device-driven cascade over queue sets (csrc/queue_set.h): parser Forward / Backward, regions, envelope Forward /
Backward / OA and region Forward run once per sequence part and Forward register class over the queues of ALL of the part's groups.  One
small search built so that the sets matter: two parts, three SSV classes that share Forward class Q = 2 (M = 70, 100, 120) and two that
share Q = 4 (M = 200, 250) -- so every set holds the queues of several groups --, and a fourth model of Q = 2 (M = 90) planted in no
sequence, whose group's queues are empty inside sets that are not.  Every kind of sequence with a domain exists short and long, so
both parts have work in both classes; a few carry two abutting partial copies (a multi-domain region: region Forward and the trace
ensemble).  The rows of the device-driven cascade must equal the host-driven one's field for field -- at 4 and at 16 hardware queues,
with tables so small that the lane falls back, and twice in one process.  test_input_gives_every_stage_work checks on the CPU (oracle
and the float64 reference of tests/fb_reference.py) that the input is what it is meant to be."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANTED = {70: 2, 100: 2, 120: 2, 200: 4, 250: 4}            # model length -> Forward register class
EMPTY_M = 90                                                 # Forward class 2, an SSV class of its own, planted nowhere
LENGTHS = sorted(list(PLANTED) + [EMPTY_M])


def profiles():
    from synthdata import synth
    prng = np.random.default_rng(2601)
    profs = [synth.random_profile(prng, M, "fs%04d" % M, "PF%05d.1" % (26000 + M)) for M in LENGTHS]
    for p in profs:
        p.stats = (-8.5 - 0.002 * p.M, 0.71, -9.5 - 0.002 * p.M, 0.71, -3.8, 0.71)
        p.ga = (25.0, 25.0)
    return profs


def world():
    """(profiles, bins, planted): bins = two lists of (name, description, protein + '*'); planted = [(model length, bin, index in the bin,
    copies)].  Background: 280 random sequences of 40 .. 900 residues.  Each planted model: a whole domain in ten short sequences (the
    domain and a few residues) and in ten long ones (890 residues), and two abutting partial copies -- nodes 1 .. 3M/4, then
    M/3 .. M -- in one short and one long sequence."""
    from synthdata import synth
    profs = profiles()
    rng = np.random.default_rng(2602)
    bins, planted = [[], []], []
    for k in range(280):
        bins[k % 2].append(("bg%d" % k, "", synth.to_text(synth.random_residues(rng, int(rng.integers(40, 901)))) + "*"))
    for n, p in enumerate(profs):
        if p.M == EMPTY_M:
            continue
        one = lambda: [synth.sample_domain(rng, p)]
        two = lambda: [synth.sample_domain(rng, p, 1, p.M * 3 // 4), synth.sample_domain(rng, p, p.M // 3, p.M)]
        # (ten whole domains per model and part: more candidates than the 8 entries a group's tables hold under CKM_CAP_SHRINK=64)
        for copies, pieces, pad in [(1, one(), 8) for _ in range(10)] + [(1, one(), 0) for _ in range(10)] + [(2, two(), 8), (2, two(), 0)]:
            body = int(sum(len(x) for x in pieces))
            left = 8 if pad else int(rng.integers(100, 200))
            right = 8 if pad else max(8, 890 - body - left)
            t = np.concatenate([synth.random_residues(rng, left)] + pieces + [synth.random_residues(rng, right)])
            assert 40 <= len(t) <= 900
            b = (n + copies) % 2
            planted.append((p.M, b, len(bins[b]), copies))
            bins[b].append(("dom%d_%dx%s_%d" % (p.M, copies, "s" if pad else "l", len(bins[b])), "", synth.to_text(t) + "*"))
    return profs, bins, planted


CODE = r'''
import sys, json, os
sys.path.insert(0, %r)
import numpy as np
from checkm_amd import _lib
from tests import common
from tests import test_gpu_float_sets as T
profs, bins, _planted = T.world()
path = common.hmm_file("float_sets", profs)
ctx = _lib.Context(0); prof = _lib.Profiles(ctx, path); seqs = _lib.Seqs(ctx, bins)
f32 = lambda v: int(np.float32(v).view(np.uint32))
runs = []
for rep in range(int(os.environ.get("CKM_TEST_REPEAT", "1"))):
    hits = _lib.search(ctx, prof, seqs)
    st = ctx.stats()
    rows = [[b, int(hits.seq[i]), int(hits.model[i]), int(hits.tlen[i]), int(hits.qlen[i]), int(hits.dom_idx[i]), int(hits.ndom[i]), int(hits.hmm_from[i]), int(hits.hmm_to[i]),
             int(hits.ali_from[i]), int(hits.ali_to[i]), int(hits.env_from[i]), int(hits.env_to[i]), f32(hits.full_score[i]), f32(hits.full_bias[i]), f32(hits.dom_score[i]),
             f32(hits.dom_bias[i]), f32(hits.acc[i]), float(hits.full_evalue[i]), float(hits.c_evalue[i]), float(hits.i_evalue[i])] for b in range(len(bins)) for i in hits.rows(b)]
    runs.append({"rows": rows, "fallback": int(st.cascade_fallback_lanes), "ssv_launches": int(st.ssv_launches),
                 "pairs": [int(st.pairs_ssv), int(st.pairs_fwd), int(st.pairs_dom), int(st.envelopes), int(st.regions_multi)]})
    hits.close()
print(json.dumps({"runs": runs}))
''' % ROOT


def _run(**extra):
    env = dict(os.environ, CKM_WORKERS="1", **extra)
    out = subprocess.run([sys.executable, "-c", CODE], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (extra, out.stderr[-3000:])
    return json.loads(out.stdout.strip().split("\n")[-1])["runs"]


@functools.lru_cache(maxsize=None)
def host_rows():
    """the host-driven cascade's rows: computed once, shared by every case, never changed"""
    host = _run(CKM_CASCADE="host")[0]
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(CKM_HW_QUEUES="4"), dict(CKM_HW_QUEUES="16")], ids=["inherited", "4_queues", "16_queues"])
def test_float_sets_equal_host_cascade(extra):
    host = host_rows()
    npl = len(PLANTED)
    assert len(host["rows"]) >= 4 * npl and host["pairs"][4] >= 2                  # every planted sequence reports; multi-domain regions are present
    dev = _run(CKM_SPLIT_MIN_PAIRS="1", **extra)[0]
    assert dev["fallback"] == 0
    # one group per (part, SSV class): six classes in two parts -- three groups share every Forward class 2 set but one group more (the empty one), two every class 4 set
    assert dev["ssv_launches"] == 2 * len(LENGTHS)
    assert dev["rows"] == host["rows"]
    assert dev["pairs"][0] == host["pairs"][0] and dev["pairs"][3] == host["pairs"][3]
    # the device decides conservatively: never fewer pairs than the exact test lets through
    assert dev["pairs"][1] >= host["pairs"][1] and dev["pairs"][2] >= host["pairs"][2]


@pytest.mark.gpu
def test_float_sets_tables_too_small_fall_back():
    tiny = _run(CKM_SPLIT_MIN_PAIRS="1", CKM_CAP_SHRINK="64")[0]
    assert tiny["fallback"] >= 1 and tiny["rows"] == host_rows()["rows"]


@pytest.mark.gpu
def test_float_sets_twice_in_one_process():
    a, b = _run(CKM_SPLIT_MIN_PAIRS="1", CKM_TEST_REPEAT="2")
    assert a["fallback"] == 0 and b["fallback"] == 0
    assert a["rows"] == b["rows"] == host_rows()["rows"]


def test_input_gives_every_stage_work():
    """On the CPU: in each of the two parts and each of the two Forward classes at least one pair reaches every one of the seven float
    stages -- it passes the Viterbi filter (parser Forward), passes F3 (parser Backward, regions), has a single-domain region (envelope
    Forward, Backward, OA) and a multi-domain one (region Forward), none of these by a margin that float32 could turn -- and no sequence
    at all passes the filters of the model that is planted nowhere."""
    from oracle import p7
    from synthdata import synth
    from tests import common
    from tests import fb_reference as fr
    profs, bins, planted = world()
    path = common.hmm_file("float_sets", profs)
    hs = p7.HmmSet(path)
    models = [fr.Model(r) for r in fr.parse_hmm(open(path).read())]
    index = dict((p.M, n) for n, p in enumerate(profs))
    # the parts, as cascade_plan.h cuts them: the longest sequences that hold a quarter of the residues, then the rest
    lens = sorted((len(r[2]) - 1 for b in bins for r in b), reverse=True)
    total, acc, lcut = sum(lens), 0, None
    for L in range(max(lens), 0, -1):
        acc += sum(x for x in lens if x == L)
        if acc >= 0.25 * total:
            lcut = L - 1
            break
    assert lcut and min(lens) <= lcut < max(lens)
    seen = set()
    for M, b, k, copies in planted:
        text = bins[b][k][2][:-1]
        dsq = p7.digitize(text)
        st = hs.stages(index[M], dsq)
        part = 0 if len(dsq) > lcut else 1
        key = (part, PLANTED[M])
        assert st.pass_msv and st.pass_bias and st.pass_vit and st.pass_fwd, (M, b, k)
        seen |= {key + ("fwd",), key + ("bwd",)}
        mocc, bt, et = fr.occupancy_c(models[index[M]].cfg(), fr.specials(len(dsq), True), dsq)[2:]
        regions, _tail = fr.regions_of(mocc, bt, et)
        for _i, _j, multi, margin in regions:
            if margin > 1e-3:                                       # (float32 posteriors are good to 1e-5 here: tests/fb_reference.py)
                seen.add(key + ("multi" if multi else "single",))
    for part in (0, 1):
        for q in sorted(set(PLANTED.values())):
            for what in ("fwd", "bwd", "single", "multi"):
                assert (part, q, what) in seen, (part, q, what)
    # the empty group is empty: no sequence passes the filters in front of the parser Forward for the model planted nowhere
    e = index[EMPTY_M]
    for b in bins:
        for _name, _desc, text in b:
            st = hs.stages(e, p7.digitize(text[:-1]))
            assert not (st.pass_msv and st.pass_bias and st.pass_vit), _name
    hs.close()
