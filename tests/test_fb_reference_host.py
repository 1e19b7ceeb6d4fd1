"""The float64 reference of the float stages (tests/fb_reference.py) held together on the host, and the oracle held to it.

No GPU: the numpy statement against the C loop, the reference's own invariants, the coverage of its world, its tolerance constants measured
again, the oracle (oracle/p7oracle.c) within those tolerances on every pair, envelope and region, and the proof that the tolerances are narrow
enough to see one wrong parameter.  tests/test_gpu_fb.py holds the kernels to the same reference."""
import collections
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import p7
from synthdata import synth
from tests import fb_reference as fb


@pytest.fixture(scope="module")
def world():
    return fb.World.get()


@pytest.fixture(scope="module")
def hs(world):
    h = p7.HmmSet(world.path)
    yield h
    h.close()


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    both_inf = np.isinf(a) & np.isinf(b) & (a == b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_inf | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))))


def _numpy_vs_c(c, L_full, dsq, label):
    bad = []
    sp, spu = fb.specials(L_full, True, c["dtype"]), fb.specials(L_full, False, c["dtype"])
    score, _fM, _fI, _xs, _ex, _exc, lxe = fb.forward_numpy(c, sp, dsq)
    f, lxe_c = fb.forward_c(c, sp, dsq)
    if not (_close(score, f) and _close(lxe[1:], lxe_c[1:])):
        bad.append((label, "forward", score, f))
    if math.isfinite(f):
        occ_n, occ_c = fb.occupancy_numpy(c, sp, dsq), fb.occupancy_c(c, sp, dsq)[2:]
        if not all(_close(a[1:], b[1:]) for a, b in zip(occ_n, occ_c)):
            bad.append((label, "occupancy"))
        n, r = fb.envelope_numpy(c, spu, dsq), fb.envelope_c(c, spu, dsq, keep=True)
        for k in ("envsc", "btotal", "null2", "oasc", "ppM", "ppI", "ppX"):
            if not _close(n[k], r[k]):
                bad.append((label, k, n[k] if np.ndim(n[k]) == 0 else None, r[k] if np.ndim(r[k]) == 0 else None))
        if n["coords"] != r["coords"] or not _close(n["gap"], r["gap"], 1e-9):
            bad.append((label, "trace", n["coords"], r["coords"], n["gap"], r["gap"]))
        if not np.array_equal(n["path"], r["path"]) or not _close(n["pp_path"], r["pp_path"]) or not _close(n["flank"], r["flank"]):
            bad.append((label, "path", n["path"], r["path"], n["flank"], r["flank"]))
    if not _close(fb.bias_numpy(c, dsq), fb.bias_c(c, dsq), 1e-12 if c["dtype"] is not np.float32 else 1e-6):
        bad.append((label, "bias"))
    return bad


def test_numpy_statement_equals_c_loop(world):
    """Every model of up to 256 nodes on its planted target, the gated model, and a sample of the longer ones on short targets."""
    jobs = []
    for pr in world.pairs:
        small = pr.M <= 256 and pr.name in ("planted", "star_mid", "r3")
        sample = pr.M in (257, 1025, 4096) and pr.name in ("r17", "deg_allx")
        if small or sample:
            jobs.append((world.model_of(pr)[1].cfg(), pr.L, pr.dsq, (pr.M, pr.gated, pr.name)))
    two = next(pr for pr in world.pairs if pr.M == 64 and pr.name == "two")             # the wide format runs the same statement
    jobs.append((world.model_of(two)[1].cfg(fb.WIDE), two.L, two.dsq, (64, "wide", "two")))
    jobs.append((world.model_of(two)[1].cfg(np.float32), two.L, two.dsq[:70], (64, "float32", "two")))
    with ThreadPoolExecutor(max_workers=8) as ex:
        bad = [b for part in ex.map(lambda j: _numpy_vs_c(*j), jobs) for b in part]
    assert len(jobs) >= 30 and not bad, bad[:10]


def test_reference_invariants(world):
    bad = []
    for pr in world.pairs:
        if math.isfinite(pr.fwd) and abs(pr.btotal - pr.fwd) > 1e-9 * max(1.0, abs(pr.fwd)):
            bad.append((pr.M, pr.name, "totals", pr.fwd, pr.btotal))
    for e in world.envs:
        r = e.ref
        if not fb.consistent(r):
            bad.append((e.M, e.name, e.ienv, e.jenv, "posteriors / totals", r["rowdev"], r["envsc"], r["btotal"]))
        if not r["oasc"] <= e.Ld + 1e-9:
            bad.append((e.M, e.name, e.ienv, e.jenv, "oasc > Ld", r["oasc"]))
        if e.wide and e.in_range:
            bad.append((e.M, e.name, e.ienv, e.jenv, "float64 left its range where float32 did not"))
    # the trace: what the walk returns besides its four end coordinates
    paths = 0
    for e in world.envs + [w for w in world.wholes if w.ref is not None and w not in world.envs]:
        r, tag = e.ref, (e.M, e.name, e.ienv, e.jenv)
        path, pp = r["path"], r["pp_path"]
        assert path.shape == (e.M + 1,) and pp.shape == (e.Ld + 1,) and path[0] == 0 and pp[0] == 0
        nodes = np.nonzero(path)[0]
        if len(nodes) == 0:
            if r["coords"] != (0, 0, 0, 0) or pp.any():
                bad.append(tag + ("no path, but coordinates or posteriors", r["coords"]))
            continue
        paths += 1
        if not np.all(np.diff(path[nodes]) > 0):
            bad.append(tag + ("residues along the path do not increase",))
        if (int(nodes[0]), int(nodes[-1]), int(path[nodes[0]]), int(path[nodes[-1]])) != r["coords"]:
            bad.append(tag + ("ends of the path", (int(nodes[0]), int(nodes[-1]), int(path[nodes[0]]), int(path[nodes[-1]])), r["coords"]))
        total = float(pp.sum()) + r["flank"]
        if not abs(total - r["oasc"]) <= 1e-9 * max(1.0, abs(r["oasc"])):
            bad.append(tag + ("sum of the path's posteriors and the flanks is not oasc", total, r["oasc"]))
        if not (np.all(pp >= 0) and np.all(pp <= 1 + 1e-12)):
            bad.append(tag + ("a posterior outside [0, 1]", float(pp.min()), float(pp.max())))
        a, b = r["coords"][2], r["coords"][3]
        if pp[:a].any() or pp[b + 1:].any() or not np.all(pp[a:b + 1] > 0):
            bad.append(tag + ("posteriors off the alignment, or none on it",))
    assert not bad, bad[:10]
    assert paths >= len(world.envs)


def test_world_coverage_and_undecided_caps(world):
    ns = collections.Counter(min(pr.nscale, 3) for pr in world.pairs)
    assert ns[0] and ns[1] and ns[3], ns
    assert sum(1 for pr in world.pairs if pr.fwd == -np.inf) >= 1
    assert any(math.isfinite(pr.fwd) for pr in world.pairs)
    single, multi, reg_und, env_all, env_und = (collections.Counter() for _ in range(5))
    for pr in world.pairs:
        for _i, _j, m, margin in pr.regions:
            (multi if m else single)[pr.q] += 1
            reg_und[pr.q] += fb.region_undecided(margin)
    for e in world.envs:
        env_all[e.q] += 1
        env_und[e.q] += e.undecided
    for q in fb.KFB_Q:
        assert single[q] >= 3, (q, single[q])
        assert env_und[q] < env_all[q] and reg_und[q] < single[q] + multi[q], q
    assert sum(multi.values()) >= 1
    nreg = sum(single.values()) + sum(multi.values())
    assert sum(reg_und.values()) <= 0.02 * nreg, (sum(reg_und.values()), nreg)
    assert sum(env_und.values()) <= 0.02 * len(world.envs), (sum(env_und.values()), len(world.envs))
    # the gated model's planted domain crosses the node whose MD is 0
    assert any(e.gated and e.ref["coords"][0] < fb.GATED_NODE < e.ref["coords"][1] for e in world.envs)


def test_tolerance_constants_are_the_measured_ones(world):
    got = fb.measure_tolerances(world)
    print("measured ratios", dict((k, v) for k, v in got.items() if k != "left_out"), "left out", len(got["left_out"]))
    for k, K in (("fwd", fb.K_FWD), ("oa", fb.K_OA), ("bias", fb.K_BIAS), ("n2", fb.K_N2), ("gap", fb.K_GAP), ("reg", fb.K_REG), ("pp", fb.K_PP)):
        assert got[k] <= K / 4.0, (k, got[k], K)
        assert fb.k_of(fb.OBSERVED[k]) == K, (k, fb.OBSERVED[k], K)
    assert fb.K_GAP < fb.K_OA
    differ = [(e.M, e.name, e.ienv, e.jenv) for e in world.envs if e.in_range and not e.undecided and
              (e.f32["coords"] != e.ref["coords"] or not np.array_equal(e.f32["path"], e.ref["path"]))]
    assert not differ, differ                      # a decided envelope's trace is the same in float32, node for node
    # what is excused is what the constants' comment says, by the exact condition, well away from its limit; and the float32 evaluation
    # hangs together on exactly the others
    assert all(e.name == "two" and e.M >= 192 and (e.ienv, e.jenv) in ((1, e.pair.L), (5, e.pair.L - 3)) for e in got["left_out"])
    assert all(abs(e.overflow) > 1.0 for e in world.envs), min(abs(e.overflow) for e in world.envs)
    assert all(e.in_range != e.excused for e in world.envs)


def test_oracle_within_tolerance(world, hs):
    def pair(pr):
        return hs.stages(world.model_of(pr)[0], pr.dsq)

    def env(e):
        return hs.envelope(world.model_of(e)[0], e.pair.dsq, e.ienv, e.jenv)
    with ThreadPoolExecutor(max_workers=8) as ex:
        stages = list(ex.map(pair, world.pairs))
        envs = list(ex.map(env, world.envs))
    bad, worst = [], collections.defaultdict(float)
    for pr, st in zip(world.pairs, stages):
        tag = ("oracle", pr.M, "gated" if pr.gated else pr.q, pr.name)
        for f, got, ref, K in (("fwd_sc", st.fwd_sc, pr.fwd, fb.K_FWD), ("bias_sc", st.bias_sc, pr.bias, fb.K_BIAS), ("null_sc", st.null_sc, pr.null, 0.0)):
            ratio = fb.score_ratio(got, ref, pr.L)
            worst[f] = max(worst[f], ratio)
            if not ratio <= K:
                bad.append(tag + (f, got, ref, ratio))
        if (st.fwd_nscale > 0) != (pr.nscale > 0) and not pr.nscale_close:
            bad.append(tag + ("fwd_nscale", st.fwd_nscale, pr.nscale))
    for e, (rc, envsc, oasc, null2, coords, _xC, _ns) in zip(world.envs, envs):
        local = (int(coords[0]), int(coords[1]), int(coords[2]) - e.ienv + 1, int(coords[3]) - e.ienv + 1)
        bad += fb.envelope_findings(e, rc == 0, envsc, oasc, null2, local, "oracle")
        if rc == 0 and e.in_range:
            for f, ratio in (("envsc", fb.score_ratio(envsc, e.ref["envsc"], e.Ld)), ("oasc", fb.score_ratio(oasc, e.ref["oasc"], e.Ld)), ("null2", fb.n2_ratio(null2, e.ref["null2"], e.Ld))):
                worst[f] = max(worst[f], ratio)
    print("largest oracle-to-reference ratios", dict(worst))
    assert not bad, bad[:10]


def test_oracle_alignments(world, hs):
    """p7o_envelope_alignment on every envelope of the world and p7o_align on every target that is aligned as a whole: refused exactly
    where excused, the path of a decided envelope node for node, its posterior line within K_PP and 0 off the alignment."""
    def env(e):
        return hs.envelope_alignment(world.model_of(e)[0], e.pair.dsq, e.ienv, e.jenv)

    def whole(e):
        return hs.align(world.model_of(e)[0], e.pair.dsq)
    with ThreadPoolExecutor(max_workers=8) as ex:
        envs = list(ex.map(env, world.envs))
        wholes = list(ex.map(whole, world.wholes))
    bad, worst, checked = [], 0.0, collections.Counter()
    for e, (rc, path, pp) in zip(world.envs, envs):
        b, ratio = fb.path_findings(e, rc == 0, path, pp, "oracle")
        bad += b
        if ratio is not None:
            worst, checked[e.q] = max(worst, ratio), checked[e.q] + 1
    decided = collections.Counter()
    for e, (rc, path) in zip(world.wholes, wholes):
        tag = ("oracle align", e.M, "gated" if e.gated else e.q, e.name)
        if e.ref is None or e.excused:                       # no path at all (the Forward total is 0), or float32 cannot hold Backward
            if rc == 0 or path.any():
                bad.append(tag + ("answered", rc))
        elif rc != 0:
            bad.append(tag + ("refused", rc, e.overflow))
        elif not e.undecided:
            decided[e.q] += 1
            if not np.array_equal(path, e.ref["path"][1:]):
                k = int(np.nonzero(path != e.ref["path"][1:])[0][0])
                bad.append(tag + ("node", k + 1, int(path[k]), int(e.ref["path"][k + 1])))
    print("largest oracle-to-reference pp ratio", worst, "paths checked", dict(checked), "whole sequences", dict(decided))
    assert not bad, bad[:10]
    assert all(checked[q] >= 3 and decided[q] >= 3 for q in fb.KFB_Q), (dict(checked), dict(decided))


def test_oracle_regions_from_search(world, hs):
    """Rows of the oracle's search against the reference's regions, where every region of the pair fails rt3 and is decided: every row's
    envelope is one of the regions (a region may lack a row: its E-value), no row twice, and ndom counts the pair's rows."""
    def rows_of(key):
        prs = [pr for pr in world.pairs if (pr.M, pr.gated) == key and fb.comparable_regions(pr)]
        return prs, hs.search([world.index[key]], [pr.dsq for pr in prs], [pr.name for pr in prs])
    with ThreadPoolExecutor(max_workers=8) as ex:
        per_model = list(ex.map(rows_of, world.keys))
    bad, checked = [], collections.Counter()
    for prs, rows in per_model:
        for s, pr in enumerate(prs):
            got = [(r.env_from, r.env_to, r.ndom) for r in rows if r.seq_idx == s]
            bad += fb.region_findings(pr, got, "oracle")
            checked[pr.q] += len(got)
    assert not bad, bad[:10]
    assert all(checked[q] >= 3 for q in fb.KFB_Q), dict(checked)


def test_tolerance_sees_one_wrong_parameter(world, hs):
    """For every class, the oracle's score under the unchanged file lies more than 10 tolerances away from the reference of
    (a) the file with MM of the middle node multiplied by 0.9 and the node's match transitions renormalised by giving MD what MM lost,
        on the planted pair: the shift is about |ln 0.9| = 0.105 nats.  (Dividing the three by their sum would give MM back all but
        0.4 % of what it lost, a shift of 0.004 nats, which ten tolerances exceed from 192 nodes on.)
    (b) the unchanged file read with the local entry distribution shifted by one node, on the class's short random targets (1, 2, 3 and 17 residues), of which at least one must see it.  The planted
        pair cannot see (b): the entry distribution is nearly flat, a full-length domain's score moves by about 0.01 nats, and ten
        tolerances of a long class's planted pair are 0.08 nats (M = 4096); the short targets' tolerance is 5e-6 nats, and they see it."""
    bad = []
    for q, lengths in fb.launch_classes():
        M = lengths[-1]
        mi = world.index[(M, False)]
        p = fb.make_profile(M)
        mid = max(1, M // 2)
        p.t[mid, 2] += 0.1 * p.t[mid, 0]
        p.t[mid, 0] *= 0.9
        changed = fb.Model(fb.parse_hmm(synth.hmm_text(p))[0])
        c = dict(world.models[mi].cfg())
        c["bm"] = np.ascontiguousarray(np.concatenate([[0.0], np.roll(c["bm"][1:], 1)]))
        seen = {}
        for what, cfg, names in (("MM x 0.9", changed.cfg(), ("planted",)), ("entry shifted", c, ("r1", "r2", "r3", "r17"))):
            for pr in (pr for pr in world.pairs if (pr.M, pr.gated) == (M, False) and pr.name in names):
                got = hs.stages(mi, pr.dsq).fwd_sc
                tol = fb.score_tol(fb.K_FWD, pr.L, pr.fwd)
                ref, _ = fb.forward_c(cfg, fb.specials(pr.L, True), pr.dsq)
                print("class", q, "M", M, what, pr.name, "shift", abs(got - ref), "tolerance", tol)
                seen[what] = max(seen.get(what, 0.0), abs(got - ref) / tol)
        bad += [(q, M, what, ratio) for what, ratio in seen.items() if not ratio > 10.0]
    assert not bad, bad
