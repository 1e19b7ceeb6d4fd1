"""The float stages on the device against the float64 reference (tests/fb_reference.py): fwd_kernel<Q>, bwd_kernel<Q>, oa_kernel<Q>, the bias
filter and region_kernel, at both edges of every Forward register class.

Unlike tests/test_gpu_scan.py this does not ask `the same bits as the oracle` but `this is Forward`: the reference shares no order, layout,
table or rescaling rule with oracle or kernels, and the tolerances are the measured constants of fb_reference.py
(tests/test_fb_reference_host.py holds the reference together and the oracle to it, without a GPU).  One library call per class."""
import collections

import numpy as np
import pytest

from checkm_amd import _lib
from tests import fb_reference as fb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gw(gpu_ctx):
    """The world on the device: one bin per model, holding that model's targets."""
    world = fb.World.get()
    bins, seq_of = [], {}
    for key in world.keys:
        recs = []
        for pr in world.pairs:
            if (pr.M, pr.gated) == key:
                seq_of[id(pr)] = sum(len(b) for b in bins) + len(recs)
                recs.append(("m%d%s_%s" % (pr.M, "g" if pr.gated else "", pr.name), "", pr.text))
        bins.append(recs)
    prof = _lib.Profiles(gpu_ctx, world.path)
    seqs = _lib.Seqs(gpu_ctx, bins)
    yield dict(ctx=gpu_ctx, world=world, prof=prof, seqs=seqs, seq_of=seq_of)
    prof.close(); seqs.close()


def _tag(pr):
    return ("kernel", pr.M, "gated" if pr.gated else pr.q, pr.name)


def test_forward_and_bias_scores(gw):
    world, bad, worst = gw["world"], [], collections.defaultdict(float)
    for q in fb.KFB_Q:
        prs = [pr for pr in world.pairs if pr.q == q]
        got = _lib.debug_stages(gw["ctx"], gw["prof"], gw["seqs"], np.array([world.model_of(pr)[0] for pr in prs]), np.array([gw["seq_of"][id(pr)] for pr in prs]))
        for pr, g in zip(prs, got):
            for f, ref, K in (("fwd_sc", pr.fwd, fb.K_FWD), ("bias_sc", pr.bias, fb.K_BIAS), ("null_sc", pr.null, 0.0)):
                ratio = fb.score_ratio(getattr(g, f), ref, pr.L)
                worst[f] = max(worst[f], ratio)
                if not ratio <= K:
                    bad.append(_tag(pr) + (f, getattr(g, f), ref, ratio))
            if (g.fwd_nscale > 0) != (pr.nscale > 0) and not pr.nscale_close:
                bad.append(_tag(pr) + ("fwd_nscale", g.fwd_nscale, pr.nscale))
    print("largest kernel-to-reference ratios", dict(worst))
    assert not bad, bad[:10]


def test_envelope_rescoring(gw):
    """ok == 1 and every figure within tolerance; the four coordinates equal unless the envelope is undecided.  The two-copy spans that
    leave float32's range (fb_reference.py, at the tolerance constants) may be refused instead: ok == 0, or every figure right."""
    world, bad, worst = gw["world"], [], collections.defaultdict(float)
    for q in fb.KFB_Q:
        envs = [e for e in world.envs if e.q == q]
        got = _lib.debug_envelopes(gw["ctx"], gw["prof"], gw["seqs"], np.array([world.model_of(e)[0] for e in envs]), np.array([gw["seq_of"][id(e.pair)] for e in envs]),
                                   np.array([e.ienv for e in envs]), np.array([e.jenv for e in envs]))
        for e, g in zip(envs, got):
            null2 = np.array(g.null2[:], dtype=np.float64)
            local = (g.hmm_from, g.hmm_to, g.ali_from - e.ienv + 1, g.ali_to - e.ienv + 1)
            bad += fb.envelope_findings(e, g.ok == 1, g.envsc, g.oasc, null2, local, "kernel")
            if g.ok == 1 and e.in_range:
                for f, ratio in (("envsc", fb.score_ratio(g.envsc, e.ref["envsc"], e.Ld)), ("oasc", fb.score_ratio(g.oasc, e.ref["oasc"], e.Ld)),
                                 ("null2", fb.n2_ratio(null2, e.ref["null2"], e.Ld))):
                    worst[f] = max(worst[f], ratio)
    print("largest kernel-to-reference ratios", dict(worst))
    assert not bad, bad[:10]


def test_region_bounds_from_search(gw):
    """The device-driven path (region_kernel and the queue-fed fwd / bwd / oa launches of the search): where every region of a pair fails
    rt3 in the reference and is decided, every row's envelope is one of the reference's regions (a region may lack a row: its E-value),
    no row twice, and ndom counts the pair's rows."""
    world = gw["world"]
    prs = [pr for pr in world.pairs if fb.comparable_regions(pr)]
    bins = [[("m%d%s_%s" % (pr.M, "g" if pr.gated else "", pr.name), "", pr.text) for pr in prs if (pr.M, pr.gated) == key] for key in world.keys]
    seqs = _lib.Seqs(gw["ctx"], bins)
    hits = _lib.search(gw["ctx"], gw["prof"], seqs, [[world.index[key]] for key in world.keys])
    rows = collections.defaultdict(list)
    for g in range(hits.n):
        rows[(int(hits.model[g]), int(hits.seq[g]))].append((int(hits.env_from[g]), int(hits.env_to[g]), int(hits.ndom[g])))
    hits.close(); seqs.close()
    order = [pr for key in world.keys for pr in prs if (pr.M, pr.gated) == key]
    bad, checked = [], collections.Counter()
    for s, pr in enumerate(order):
        got = rows.get((world.model_of(pr)[0], s), [])
        bad += fb.region_findings(pr, got, "kernel")
        checked[pr.q] += len(got)
    assert not bad, bad[:10]
    assert all(checked[q] >= 3 for q in fb.KFB_Q), dict(checked)
