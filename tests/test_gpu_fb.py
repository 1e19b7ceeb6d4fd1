"""The float stages on the device against the float64 reference (tests/fb_reference.py): fwd_kernel<Q>, bwd_kernel<Q>, oa_kernel<Q> with the
path it traces and its posterior line, ckm_align, the bias filter and region_kernel, at both edges of every Forward register class; and the
trace ensemble (kernels_ens.hip) at the same edges against the oracle, which is its only reference.

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


def test_envelope_paths_and_posteriors(gw):
    """The OA path itself (what ckm_align and the alignments of ckm_hits_write_alignments are made of), of every envelope of the world:
    refused exactly where the reference says float32 cannot hold Backward; where the envelope is decided, the residue of every one of
    the M match nodes equals the reference's, and the posterior line is within K_PP 2^-24 on the alignment and 0 off it.

    What a wrong traceback would do here: `path[k] = i` written to path[k + 1] shifts every residue of a decided path by one node, and
    the node-for-node comparison names the first one (in every class: each has at least three decided paths); lds_cell<Q> evaluated for
    a neighbouring class reads the candidates of other nodes from the lane-striped OA rows, so the walk leaves the reference's path in
    a domain that spans the model -- the last two assertions make sure that the largest classes have such a path through node M of
    the M = 64 Q model, the last cell of the last lane, and one through an insert state -- and where it only reads ppres from the
    wrong cell, the posterior line misses K_PP: neighbouring cells of a planted domain differ by the order of the posterior itself."""
    world, bad, worst = gw["world"], [], 0.0
    checked, last_node, inserts = (collections.Counter() for _ in range(3))
    for q in fb.KFB_Q:
        envs = [e for e in world.envs if e.q == q]
        ok, paths, pps = _lib.debug_envelope_paths(gw["ctx"], gw["prof"], gw["seqs"], np.array([world.model_of(e)[0] for e in envs]),
                                                   np.array([gw["seq_of"][id(e.pair)] for e in envs]), np.array([e.ienv for e in envs]), np.array([e.jenv for e in envs]))
        for e, o, path, pp in zip(envs, ok, paths, pps):
            assert path.shape == (e.M,) and pp.shape == (e.Ld + 1,)
            found, ratio = fb.path_findings(e, o == 1, path, pp, "kernel")
            bad += found
            if o == 0 and (path.any() or pp.any()):
                bad.append(_tag(e.pair) + (e.ienv, e.jenv, "refused, but a path was written"))
            if ratio is not None:
                worst, checked[q] = max(worst, ratio), checked[q] + 1
                nodes = np.nonzero(path)[0]
                last_node[q] += int(e.M == 64 * q and path[e.M - 1] > 0)
                inserts[q] += int(np.any((np.diff(nodes) == 1) & (np.diff(path[nodes]) > 1)))      # residues between two neighbouring match nodes
    print("largest kernel-to-reference pp ratio", worst, "paths checked", dict(checked))
    assert not bad, bad[:10]
    assert all(checked[q] >= 3 for q in fb.KFB_Q), dict(checked)
    assert all(last_node[q] >= 1 and inserts[q] >= 1 for q in fb.KFB_Q[-2:]), (dict(last_node), dict(inserts))


def test_align_whole_sequences(gw):
    """ckm_align on the targets of fb_reference.WHOLE_NAMES against the unihit span (1, L) of the reference: the row is the path where that
    is decided; it is all zero exactly where the reference excuses the span (float32 cannot hold its Backward) or the target has no path
    at all (star_only: the Forward total is 0), and nowhere else; a sequence without residues keeps its row of zeros."""
    world, bad, decided = gw["world"], [], collections.Counter()
    for q in fb.KFB_Q:
        es = [e for e in world.wholes if e.q == q]
        rows = _lib.align(gw["ctx"], gw["prof"], gw["seqs"], np.array([world.model_of(e)[0] for e in es]), np.array([gw["seq_of"][id(e.pair)] for e in es]))
        for e, row in zip(es, rows):
            assert row.shape == (e.M,)
            if e.ref is None or e.excused:
                if row.any():
                    bad.append(_tag(e.pair) + ("aligned where it must be refused", e.overflow))
            elif not row.any():
                bad.append(_tag(e.pair) + ("no column where the reference has a path", e.overflow))
            elif not e.undecided:
                decided[q] += 1
                if not np.array_equal(row, e.ref["path"][1:]):
                    k = int(np.nonzero(row != e.ref["path"][1:])[0][0])
                    bad.append(_tag(e.pair) + ("node", k + 1, int(row[k]), int(e.ref["path"][k + 1])))
    assert not bad, bad[:10]
    assert all(decided[q] >= 3 for q in fb.KFB_Q), dict(decided)
    assert set(e.name for e in world.wholes) == set(fb.WHOLE_NAMES) and any(e.ref is None for e in world.wholes) and any(e.excused for e in world.wholes)
    # a sequence without residues between two others, in one call
    pr = next(pr for pr in world.pairs if pr.M == 64 and pr.name == "planted")
    want = next(e for e in world.wholes if e.pair is pr)
    seqs = _lib.Seqs(gw["ctx"], [[("first", "", pr.text), ("empty", "", ""), ("last", "", pr.text)]])
    rows = _lib.align(gw["ctx"], gw["prof"], seqs, [world.model_of(pr)[0]] * 3, [0, 1, 2])
    seqs.close()
    assert not want.undecided and not rows[1].any()
    assert np.array_equal(rows[0], want.ref["path"][1:]) and np.array_equal(rows[2], want.ref["path"][1:])


def test_trace_ensembles_at_class_edges(gw):
    """The trace ensemble (kernels_ens.hip over the cell-major Forward matrix) of every model of the world, device against oracle bit for
    bit as tests/test_gpu_scan.py::test_trace_ensemble_identical asserts it: the segments of all 200 traces, the null2 sums' bit
    patterns and the clustered envelopes, on the regions (1, L) and (3, L - 2) of fb_reference.ensemble_target (its seed is documented
    there).  The traces are samples, not a closed-form quantity: the oracle is their only reference."""
    from oracle import p7
    from tests import common
    world = gw["world"]
    texts = [fb.ensemble_target(p, gated) for (_M, gated), p in zip(world.keys, world.profs)]
    seqs = _lib.Seqs(gw["ctx"], [[("ens%d%s" % (M, "g" if gated else ""), "", tx) for (M, gated), tx in zip(world.keys, texts)]])
    hs = p7.HmmSet(world.path)
    ran, two = collections.Counter(), collections.Counter()
    try:
        for m, ((M, gated), tx) in enumerate(zip(world.keys, texts)):
            dsq, q = p7.digitize(tx), fb.class_of(M)
            L = len(dsq)
            for ireg, jreg in ((1, L), (3, L - 2)):
                tag = (M, "gated" if gated else q, ireg, jreg)
                rc, n2o, sego, nsego, envo = hs.region_ensemble(m, dsq, ireg, jreg)
                if rc != 0:                                   # the oracle refuses the region: so must the device
                    with pytest.raises(Exception):
                        _lib.debug_region(gw["ctx"], gw["prof"], seqs, m, m, ireg, jreg)
                    continue
                n2g, segg, nsegg, envg = _lib.debug_region(gw["ctx"], gw["prof"], seqs, m, m, ireg, jreg)
                assert (nsego == nsegg).all(), (tag, np.nonzero(nsego != nsegg)[0][:5])
                for t in range(200):
                    assert (sego[t, :nsego[t]] == segg[t, :nsegg[t]]).all(), (tag, t)
                assert (common.float_bits(n2o) == common.float_bits(n2g)).all(), (tag, np.nonzero(n2o != n2g)[0][:5])
                assert envo.tolist() == envg.tolist(), (tag, envo.tolist(), envg.tolist())
                ran[(q, ireg)] += 1
                two[q] += int(nsego.max() >= 2)
    finally:
        seqs.close(); hs.close()
    assert all(ran[(q, 1)] >= 1 and ran[(q, 3)] >= 1 for q in fb.KFB_Q), dict(ran)          # every class ran both regions
    assert all(two[q] >= 1 for q in fb.KFB_Q[1:]), dict(two)                               # ... and some trace sampled two segments: the target tests something


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
