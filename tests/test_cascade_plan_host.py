"""The search's host-side plan (csrc/cascade_plan.h): which pairs a lane owns, where every bin's length-sorted order is cut into parts, the
SSV block tables of both cascades and their groups, the groups' capacities, the verdicts before any launch and what a drained search
teaches the divisors and floors.  The header is pure host code: tests/native/cascade_plan_check.cpp is compiled with AddressSanitizer and
UBSan, run as a child process on a case file, and its plan is held against a restatement of the rules in Python.  No device needed."""
import json
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

NVC, NFC, CC_SIZE = 26, 12, 128                        # dev_types.h
CC = dict(CAND=0, NORES=1, FWORK=2, EWORK=3, RWORK=4, PASS=5, REG=6, EVENTS=7, STATUS=8, EVENTS_E=9, VQ=16, VXQ=16 + NVC, FQ=16 + 2 * NVC,
          BQ=16 + 2 * NVC + NFC, EQ=16 + 2 * NVC + 2 * NFC, RQ=16 + 2 * NVC + 3 * NFC)
CS_RWORK = 16
SSV_NONE = 65
GO, NO_PAIRS, OVER_BUDGET, TOO_MANY_GROUPS = 0, 1, 2, 3
CAP_MAX = 0x7ffffff0
CAPS0 = dict(fwork=0, ework=0, rwork=0, **{"pass": 0}, reg=0, events_f=0, events_e=0, seen_rwork=0, hens=0, div_cand=12, div_nores=48, div_fwork=160,
             div_ework=256, div_rwork=32768, fl_cand=4096, fl_nores=2048, fl_fwork=2048, fl_ework=1024, fl_rwork=256, ws_per_cell=11.0, z1_per_pair=64.0)
CAP_FIELDS = list(CAPS0)
KINDS = [("cand", "div_cand", "fl_cand"), ("nores", "div_nores", "fl_nores"), ("f", "div_fwork", "fl_fwork"), ("e", "div_ework", "fl_ework"),
         ("r", "div_rwork", "fl_rwork")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("cascade_plan")
    exe = str(d / "cascade_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "cascade_plan_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


# ---- cases ------------------------------------------------------------------------------------------------------------------------
class Case:
    """Sequences in bins (every bin's order is longest first), models with their bins, the lane's models, the options of a call."""

    def __init__(self, bin_lens, models, lane, pair_budget=1 << 29, split_min=1, shrink=1, share=None, ws_budget=8 << 30, ws_floats=(1 << 30) // 4,
                 empty_bins=(), blocks=True):
        self.len, self.order, self.lo, self.hi = [], [], [], []
        for b, lens in enumerate(bin_lens):
            ids = list(range(len(self.len), len(self.len) + len(lens)))
            self.len += lens
            self.lo.append(len(self.order))
            self.order += sorted(ids, key=lambda q: -self.len[q])
            self.hi.append(self.lo[-1] if b in empty_bins else len(self.order))      # (a lane's length class may hold nothing of a bin)
        self.res = [sum(self.len[q] for q in self.order[lo:hi]) for lo, hi in zip(self.lo, self.hi)]
        self.models, self.lane = models, lane                 # models: dicts cls, per_block, M, fbQ, vit, vitx, fb, bins
        self.pair_budget, self.split_min, self.shrink, self.share, self.ws_budget, self.ws_floats, self.blocks = pair_budget, split_min, shrink, share, ws_budget, ws_floats, blocks

    def L(self, k):
        return self.len[self.order[k]]

    def text(self, caps=None, cnt=(), tops=None):
        t = ["opt %d %d %d %s" % (self.pair_budget, self.split_min, self.shrink, self.share if self.share is not None else "-"),
             "ws %d %d" % (self.ws_budget, self.ws_floats), "len %d %s" % (len(self.len), " ".join(map(str, self.len))),
             "order %d %s" % (len(self.order), " ".join(map(str, self.order))),
             "bins %d %s" % (len(self.lo), " ".join("%d %d %d" % x for x in zip(self.lo, self.hi, self.res))), "models %d" % len(self.models)]
        for m in self.models:
            t.append("%d %d %d %d %d %d %d %d %s" % (m["cls"], m["per_block"], m["M"], m["fbQ"], m["vit"], m["vitx"], m["fb"], len(m["bins"]), " ".join(map(str, m["bins"]))))
        t.append("lane %d %s" % (len(self.lane), " ".join(map(str, self.lane))))
        if caps:
            t.append("caps " + " ".join(repr(caps[f]) for f in CAP_FIELDS))
        t += ["cnt %d %d %d" % c for c in cnt]
        if tops:
            t.append("tops %d %d %d %d" % tuple(tops))
        t.append("blocks %d" % self.blocks)
        return "\n".join(t) + "\n"


def run(harness, case, **kw):
    exe, d = harness
    path = str(d / "case.txt")
    open(path, "w").write(case.text(**kw))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return json.loads(out.stdout)


def model(cls, per_block, M, bins, fbQ=None, vit=0, vitx=12, fb=0):
    return dict(cls=cls, per_block=per_block, M=M, fbQ=fbQ if fbQ is not None else (M + 63) // 64, vit=vit, vitx=vitx, fb=fb, bins=bins)


def mixed_case(**kw):
    """Four bins of a few dozen sequences: bin 2 holds short sequences only (none of them in the long part), bin 3 is empty for this lane.
    An 8-lane class (103) with two models, two 16-lane classes (5, 12), a model without an SSV instance, and a model whose bins are all empty."""
    r = random.Random(5)
    bins = [[r.randrange(60, 900) for _ in range(37)], [r.randrange(40, 700) for _ in range(29)], [r.randrange(20, 45) for _ in range(23)], [r.randrange(50, 500) for _ in range(11)]]
    bins[0][3] = bins[0][9] = bins[1][4] = 555                          # equal lengths: the stable orders show
    models = [model(103, 16, 40, [0, 1, 2], vit=2, vitx=14, fb=0), model(103, 16, 47, [1], vit=2, vitx=14, fb=1), model(5, 8, 300, [0, 2], vit=7, vitx=16, fb=4),
              model(SSV_NONE, 4, 2500, [0, 1], vit=24, vitx=24, fb=9), model(12, 8, 700, [2], vit=9, vitx=19, fb=6), model(7, 8, 400, [3], vit=8, vitx=17, fb=5)]
    return Case(bins, models, [3, 0, 5, 2, 1, 4], empty_bins=(3,), **kw)


def dense_case(**kw):
    """The shape of test_queue_adaptation_reaches_a_fixed_point: 36000 pairs in two groups of 24000 and 12000, below split_min (one part)"""
    r = random.Random(9)
    bins = [[r.randrange(30, 400) for _ in range(500)]]
    models = [model(103, 128, 45, [0], vit=2, vitx=14, fb=0) for _ in range(48)] + [model(5, 64, 300, [0], vit=7, vitx=16, fb=4) for _ in range(24)]
    kw.setdefault("split_min", 2000000)
    return Case(bins, models, list(range(72)), blocks=False, **kw)


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------
def code(cls):
    """the SSV launch class as a code that grows with the length of the models: 8-lane classes 100 + Q8 -> Q8, 16-lane Q -> 40 + Q"""
    return cls - 100 if cls >= 100 else 40 + cls


def lane_models(c, i0=0, budget=None):
    """(model, base of its pairs, pairs) for the lane's models from i0 on that have pairs; a chunk ends in front of the model that would
    take it over the budget, but always holds one model"""
    out, total, i = [], 0, i0
    while i < len(c.lane):
        m = c.lane[i]
        n = sum(c.hi[b] - c.lo[b] for b in c.models[m]["bins"])
        if n and budget is not None and out and total + n > budget:
            break
        if n:
            out.append((m, total, n))
            total += n
        i += 1
    return out, total, i


def shares(text):
    """the shares of the residues of all parts but the last: a comma-separated list read up to the first item that is no number;
    values outside (0, 1) are left out.  Unset: a quarter."""
    if text is None:
        return [0.25]
    out = []
    for tok in text.split(","):
        m = re.match(r"\s*[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", tok)
        if not m:
            break
        if 0.0 < float(m.group(0)) < 1.0:
            out.append(float(m.group(0)))
        if m.end() != len(tok):
            break
    return out


def parts(c, total_pairs):
    """Lcuts (descending part boundaries: lengths > Lcut | <= Lcut) and cut[part][bin] .. cut[part + 1][bin]"""
    sh, lcuts = shares(c.share), []
    if total_pairs >= c.split_min and sh:
        lens = sorted((c.L(k) for lo, hi in zip(c.lo, c.hi) for k in range(lo, hi)), reverse=True)
        total, acc, si, want = sum(lens), 0, 0, sh[0]
        for L in range(max(c.len), 0, -1):              # walk the lengths down; a share is reached where the residues of the lengths >= L hold it
            if si >= len(sh):
                break
            acc += sum(x for x in lens if x == L)
            if acc >= want * total:
                if L - 1 > 0 and (not lcuts or L - 1 < lcuts[-1]):
                    lcuts.append(L - 1)
                si += 1
                if si < len(sh):
                    want += sh[si]
    cut = [list(c.lo)]
    for lc in lcuts:
        cut.append([lo + sum(1 for k in range(lo, hi) if c.L(k) > lc) for lo, hi in zip(c.lo, c.hi)])
    cut.append(list(c.hi))
    return lcuts, cut


def runs_of(c, mws, cut):
    """every non-empty (model, bin, part) in that order: (part, model, first position, count, index of its first pair)"""
    out = []
    for m, base, _n in mws:
        pb = base
        for b in c.models[m]["bins"]:
            for part in range(len(cut) - 1):
                a0, a1 = cut[part][b], cut[part + 1][b]
                if a1 > a0:
                    out.append((part, m, a0, a1 - a0, pb + a0 - c.lo[b]))
            pb += c.hi[b] - c.lo[b]
    return out


def dev_table(c, mws, cut):
    """groups by key = part * 1000 + code(class), ascending; in a group the runs by the length of their first sequence (longest first,
    ties in the order found), then the first block of every run, the second of every run, ..."""
    by_key = {}
    for part, m, first, count, pair0 in runs_of(c, mws, cut):
        by_key.setdefault(part * 1000 + code(c.models[m]["cls"]), []).append((m, first, count, pair0))
    blocks, groups = [], []
    for key in sorted(by_key):
        rv = sorted(by_key[key], key=lambda r: -c.L(r[1]))
        pb, start, a = c.models[rv[0][0]]["per_block"], len(blocks), 0
        while any(a < r[2] for r in rv):
            blocks += [[m, first + a, min(pb, count - a), pair0 + a] for m, first, count, pair0 in rv if a < count]
            a += pb
        groups.append([key, start, len(blocks) - start])
    return groups, blocks


def host_table(c, mws):
    """one group per SSV class, ascending by the class itself; its blocks, cut from every (model, bin) in turn, longest first sequence
    first (ties in the order cut)"""
    by_cls = {}
    for _part, m, first, count, pair0 in runs_of(c, mws, [c.lo, c.hi]):
        pb = c.models[m]["per_block"]
        by_cls.setdefault(c.models[m]["cls"], []).extend([m, first + a, min(pb, count - a), pair0 + a] for a in range(0, count, pb))
    blocks, groups = [], []
    for cls in sorted(by_cls):
        groups.append([cls, len(blocks), len(by_cls[cls])])
        blocks += sorted(by_cls[cls], key=lambda w: -c.L(w[1]))
    return groups, blocks


def subs_of(c, mws, cut, groups):
    """per group: class, pairs, the Viterbi and Forward classes and the longest of its models"""
    subs = {g[0]: dict(Q=(100 + g[0] % 1000 if g[0] % 1000 < 40 else g[0] % 1000 - 40), maxM=0, first=g[1], nblocks=g[2], pairs=0, vit=set(), fb=set()) for g in groups}
    for m, _base, _n in mws:
        md = c.models[m]
        for part in range(len(cut) - 1):
            sb = subs.get(part * 1000 + code(md["cls"]))
            if sb is None:
                continue
            sb["pairs"] += sum(cut[part + 1][b] - cut[part][b] for b in md["bins"])
            sb["vit"] |= {md["vit"], md["vitx"]}
            sb["fb"].add(md["fb"])
            sb["maxM"] = max(sb["maxM"], md["M"])
    return [subs[g[0]] for g in groups]


def capof(pairs, div, floor, shrink):
    """max(share, floor), the share being pairs / divisor; CKM_CAP_SHRINK=n: a share n times smaller, and 8 for every floor"""
    return min(max(8 if shrink > 1 else floor, pairs // (div * shrink)), CAP_MAX)


def size_tables(subs, caps, shrink):
    """fills the groups' capacities and offsets; returns the grown shared capacities"""
    cp, tot = dict(caps), dict(cand=0, nores=0, f=0, e=0, r=0)
    for sb in subs:
        for kind, div, fl in KINDS:
            sb["cap_" + kind] = capof(sb["pairs"], cp[div], cp[fl], shrink)
        if sb["Q"] == SSV_NONE:
            sb["cap_nores"] = min(sb["pairs"] + 64, CAP_MAX)            # no SSV for these models: every pair is recomputed exactly
        sb["o_cand"], sb["o_nores"], sb["o_vq"] = tot["cand"], tot["nores"], tot["cand"] * NVC
        sb["o_f"], sb["o_e"], sb["o_r"] = tot["f"] * NFC, tot["e"] * NFC, tot["r"] * NFC
        for kind in tot:
            tot[kind] += sb["cap_" + kind]
    def grow(f, want):
        cp[f] = max(cp[f], min(want, 0xfffffff0))
    grow("fwork", tot["f"]), grow("ework", tot["e"]), grow("rwork", tot["r"])
    grow("pass", max(1 << 13, tot["e"])), grow("reg", cp["ework"] + cp["rwork"])
    grow("events_f", max(1 << 18, cp["fwork"] * 16)), grow("events_e", max(1 << 16, cp["ework"] * 16))
    cp["hens"] = max(cp["hens"], min(cp["rwork"], 4 * cp["seen_rwork"] + 8192) * (256 + 200 * 16 * 4 + 1024))
    return cp, tot


def learn(subs, caps, cnt, shrink):
    """what a drained search teaches: (fits, overflow records, capacities).  cnt: {(block, counter): value}"""
    cp, over, halved = dict(caps), [], set()
    get = lambda b, k: cnt.get((b, k), 0)
    status = get(0, CC["STATUS"])
    cp["seen_rwork"] = max(cp["seen_rwork"], get(0, CC["RWORK"]))
    for what, k in (("fwork", "FWORK"), ("ework", "EWORK"), ("rwork", "RWORK"), ("pass", "PASS"), ("reg", "REG"), ("events_f", "EVENTS"), ("events_e", "EVENTS_E")):
        n = get(0, CC[k])
        if n > cp[what]:                    # a shared table: what was asked for, a quarter more and 1024
            over.append([what, -1, -1, n, cp[what]])
            cp[what] = min(n + n // 4 + 1024, 0xfffffff0)

    def teach(kind, pairs, want):
        _k, div, fl = KINDS[kind]
        w = want + want // 4 + 16
        # the divisor halves at most once per search and kind, and only where the share was the larger term
        if (pairs // max(1, cp[div] * shrink) >= cp[fl] or shrink > 1) and kind not in halved:
            cp[div] = max(1, cp[div] // 2)
            halved.add(kind)
        if shrink > 1:
            return                          # (shrunk tables: the floors do not move)
        cp[fl] = min(max(cp[fl], w), 1 << 14)
        if w > 1 << 14:                     # more than a floor may become: the share has to give the entries ...
            if pairs // w >= 1:
                cp[div] = min(cp[div], pairs // w)
            else:                           # ... unless the group asks for more entries than it has pairs
                cp[div], cp[fl] = 1, min(max(cp[fl], w), 1 << 20)

    for g, sb in enumerate(subs):
        b = 1 + g
        if get(b, CC["CAND"]) > sb["cap_cand"]:
            over.append(["cand", g, -1, get(b, CC["CAND"]), sb["cap_cand"]])
            teach(0, sb["pairs"], get(b, CC["CAND"]))
        if get(b, CC["NORES"]) > sb["cap_nores"]:
            over.append(["nores", g, -1, get(b, CC["NORES"]), sb["cap_nores"]])
            if sb["Q"] != SSV_NONE:
                teach(1, sb["pairs"], get(b, CC["NORES"]))
        for k in range(NVC):
            v = max(get(b, CC["VQ"] + k), get(b, CC["VXQ"] + k))
            if v > sb["cap_cand"]:
                over.append(["vq", g, k, v, sb["cap_cand"]])
                teach(0, sb["pairs"], v)
        for k in range(NFC):
            f = max(get(b, CC["FQ"] + k), get(b, CC["BQ"] + k))
            if f > sb["cap_f"]:
                over.append(["fq", g, k, f, sb["cap_f"]])
                teach(2, sb["pairs"], f)
            for what, q, kind in (("eq", "EQ", 3), ("rq", "RQ", 4)):
                n = get(b, CC[q] + k)
                if n > sb["cap_" + "er"[kind - 3]]:
                    over.append([what, g, k, n, sb["cap_" + "er"[kind - 3]]])
                    teach(kind, sb["pairs"], n)
    if status & CS_RWORK:
        cp["hens"] *= 2
    return status == 0 and not over, over, cp


def check_table(c, mws, groups, blocks, total_pairs):
    """every pair of the lane in exactly one block, at its own index; no block larger than its class allows; the groups tile the table"""
    index = {}
    for m, base, _n in mws:
        pb = base
        for b in c.models[m]["bins"]:
            for k in range(c.lo[b], c.hi[b]):
                index[(m, k)] = pb + k - c.lo[b]
            pb += c.hi[b] - c.lo[b]
    assert len(index) == total_pairs
    seen = []
    for m, start, count, pair_start in blocks:
        assert 1 <= count <= c.models[m]["per_block"]
        assert [index[(m, start + a)] for a in range(count)] == list(range(pair_start, pair_start + count))
        seen += range(pair_start, pair_start + count)
    assert sorted(seen) == list(range(total_pairs))
    assert [g[0] for g in groups] == sorted(set(g[0] for g in groups))
    at = 0
    for _key, first, n in groups:
        assert first == at and n > 0
        at += n
    assert at == len(blocks)


# ---- pairs and parts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share,nparts", [(None, 2), ("0.25", 2), ("0.2,0.4", 3), ("0.3,x", 2), ("x", 1), ("1.5,0.1", 2)])
def test_pairs_parts_and_both_block_tables(harness, share, nparts):
    c = mixed_case(share=share)
    got = run(harness, c)
    mws, total, _ = lane_models(c)
    assert [m for m, _b, _n in mws] == [3, 0, 2, 1, 4]                  # model 5's bins are all empty: skipped
    assert got["verdict"] == GO and got["total_pairs"] == total and got["mws"] == [list(x) for x in mws]
    lcuts, cut = parts(c, total)
    assert got["nparts"] == nparts == len(lcuts) + 1 and got["Lcuts"] == lcuts and got["Lcut"] == (lcuts[0] if lcuts else 0) and got["cut"] == cut
    for row, nxt in zip(got["cut"], got["cut"][1:]):                    # monotone, within [lo, hi]
        assert all(lo <= a <= b <= hi for lo, a, b, hi in zip(c.lo, row, nxt, c.hi))
    for k, lc in enumerate(lcuts):                                      # the boundary is a length: longer sequences in front of it, the others behind
        for b in range(len(c.lo)):
            assert all(c.L(q) > lc for q in range(c.lo[b], got["cut"][k + 1][b])) and all(c.L(q) <= lc for q in range(got["cut"][k + 1][b], c.hi[b]))
    # the device-driven table
    groups, blocks = dev_table(c, mws, cut)
    assert got["dev"]["groups"] == groups and got["dev"]["blocks"] == blocks
    check_table(c, mws, got["dev"]["groups"], got["dev"]["blocks"], total)
    keys = [g[0] for g in groups]
    if nparts > 1:
        # model 4 has the short bin alone: its class has no group in the long part and one in a later part
        assert cut[1][2] == c.lo[2] and code(12) not in keys and any(k >= 1000 and k % 1000 == code(12) for k in keys)
    assert {k % 1000 for k in keys} == {3, 45, 52, 105}                   # 8-lane 103, 16-lane 5 and 12, none
    assert got["dev"]["pairs"] == total and got["dev"]["residues"] == sum(c.res[b] for m, _b, _n in mws for b in c.models[m]["bins"])
    assert got["dev"]["cells"] == sum(c.res[b] * c.models[m]["M"] for m, _b, _n in mws for b in c.models[m]["bins"])
    # long part first, inside a part the heaviest class first
    want_order = [g for part in range(nparts) for g in reversed(range(len(keys))) if keys[g] // 1000 == part]
    assert got["order"] == want_order
    # the key: the cuts and the tag 0xde in it, the models and their bins behind them
    tail = [x for m, _b, _n in mws for x in [0xffffffff + m] + c.models[m]["bins"]]
    assert got["key"] == [11, 22, c.pair_budget, got["Lcut"], 7, 0xde] + [0xc0000000 + lc for lc in lcuts] + tail
    assert got["resident"] == 1 and got["resident_blocks"] == 0 and got["resident_same"] == 1
    # the host-driven table: one chunk
    assert len(got["host"]) == 1
    h = got["host"][0]
    hg, hb = host_table(c, mws)
    assert h["mws"] == got["mws"] and h["next"] == len(c.lane) and h["groups"] == hg and h["blocks"] == hb
    assert [g[0] for g in hg] == [5, 12, SSV_NONE, 103]
    check_table(c, mws, h["groups"], h["blocks"], total)
    assert h["key"] == [11, 22, c.pair_budget, len(c.lane), 7] + tail and h["key"] != got["key"]
    assert (h["pairs"], h["residues"], h["cells"]) == (got["dev"]["pairs"], got["dev"]["residues"], got["dev"]["cells"])
    # the groups' demands
    subs = subs_of(c, mws, cut, groups)
    for sb, g in zip(subs, got["subs"]):
        assert (g["Q"], g["maxM"], g["first"], g["nblocks"], g["pairs"], set(g["vit"]), set(g["fb"])) == \
            (sb["Q"], sb["maxM"], sb["first"], sb["nblocks"], sb["pairs"], sb["vit"], sb["fb"])
    assert sum(g["pairs"] for g in got["subs"]) == total


def test_below_split_min_there_is_one_part(harness):
    total = lane_models(mixed_case())[1]
    one = run(harness, mixed_case(split_min=total + 1))
    assert one["nparts"] == 1 and one["Lcuts"] == [] and one["Lcut"] == 0 and len(one["cut"]) == 2
    assert all(g[0] < 1000 for g in one["dev"]["groups"])
    assert run(harness, mixed_case(split_min=total))["nparts"] == 2


def test_host_driven_chunks_under_the_pair_budget(harness):
    """a chunk takes the models up to the budget, one model at least; every chunk has its own table and key"""
    c = mixed_case()
    mws, total, _ = lane_models(c)
    c.pair_budget = max(n for _m, _b, n in mws) + 1
    got = run(harness, c)
    assert got["verdict"] == OVER_BUDGET and got["dev"]["nblocks"] == 0
    i0, chunks = 0, []
    while i0 < len(c.lane):
        cm, ct, i0 = lane_models(c, i0, c.pair_budget)
        if cm:
            chunks.append((cm, ct, i0))
    assert len(chunks) > 1 and len(got["host"]) == len(chunks)
    for h, (cm, ct, nxt) in zip(got["host"], chunks):
        hg, hb = host_table(c, cm)
        assert h["next"] == nxt and h["total_pairs"] == ct and h["mws"] == [list(x) for x in cm] and h["groups"] == hg and h["blocks"] == hb
        check_table(c, cm, h["groups"], h["blocks"], ct)
        assert h["key"][:5] == [11, 22, c.pair_budget, nxt, 7]


# ---- verdicts ----------------------------------------------------------------------------------------------------------------------------
def test_verdicts(harness):
    total = lane_models(mixed_case())[1]
    assert run(harness, mixed_case(pair_budget=total))["verdict"] == GO
    assert run(harness, mixed_case(pair_budget=total - 1))["verdict"] == OVER_BUDGET        # budget exceeded by one pair
    nothing = mixed_case()
    nothing.lane = [5]
    got = run(harness, nothing)
    assert got["verdict"] == NO_PAIRS and got["total_pairs"] == 0 and got["host"] == []
    nothing.lane = []
    assert run(harness, nothing)["verdict"] == NO_PAIRS


@pytest.mark.parametrize("nclasses,short_only,ngroups,verdict", [(96, 0, 192, GO), (96, 1, 193, TOO_MANY_GROUPS), (97, 0, 194, TOO_MANY_GROUPS)])
def test_more_than_192_groups(harness, nclasses, short_only, ngroups, verdict):
    """class codes used directly: 96 classes over two parts are 192 groups, the most a search may have (one event per group).  One more class
    whose only bin holds short sequences alone has no group in the long part: 193 groups.  97 classes over two parts are 194."""
    pool = [100 + q for q in range(1, 40)] + list(range(1, 66))
    classes = pool[:nclasses]
    models = [model(cls, 4, 50, [0]) for cls in classes] + [model(cls, 4, 50, [1]) for cls in pool[nclasses:nclasses + short_only]]
    assert len(set(code(m["cls"]) for m in models)) == len(models) == nclasses + short_only
    c = Case([[900, 800, 30, 20], [25, 15]], models, list(range(len(models))))
    got = run(harness, c)
    assert got["nparts"] == 2 and got["Lcuts"] == [899] and got["cut"][1] == [1, 4]            # bin 1 has nothing in the long part
    assert len(got["dev"]["groups"]) == ngroups == 2 * nclasses + short_only and got["verdict"] == verdict
    if verdict == GO:
        assert len(got["subs"]) == 192 and sorted(got["order"]) == list(range(192))


# ---- capacities ------------------------------------------------------------------------------------------------------------------------------
def shares_case(**kw):
    """60000 pairs of an 8-lane class (its shares of candidates and Forward items above the floors), 4000 of a 16-lane class and 1000 without SSV"""
    r = random.Random(3)
    bins = [[r.randrange(30, 400) for _ in range(1000)]]
    models = [model(103, 128, 45, [0], fbQ=1) for _ in range(60)] + [model(5, 64, 300, [0], fbQ=6, vit=7, fb=4) for _ in range(4)] + [model(SSV_NONE, 16, 2500, [0], fbQ=48, vit=24, vitx=24, fb=10)]
    kw.setdefault("split_min", 2000000)
    return Case(bins, models, list(range(65)), blocks=False, **kw)


def check_sizes(c, got, caps_in, shrink=1):
    mws, total, _ = lane_models(c)
    lcuts, cut = parts(c, total)
    subs = subs_of(c, mws, cut, got["dev"]["groups"])
    cp, tot = size_tables(subs, caps_in, shrink)
    for sb, g in zip(subs, got["subs"]):
        for f in ("cap_cand", "cap_nores", "cap_f", "cap_e", "cap_r", "o_cand", "o_nores", "o_vq", "o_f", "o_e", "o_r"):
            assert g[f] == sb[f], f
        assert g["o_vq"] == g["o_cand"] * NVC
    assert [got["tot_" + k] for k in ("cand", "nores", "f", "e", "r")] == [tot[k] for k in ("cand", "nores", "f", "e", "r")]
    for f in CAP_FIELDS[:19]:
        assert got["caps"][f] == cp[f], f
    # the offsets tile the tables
    for cap, off, per in (("cap_cand", "o_cand", 1), ("cap_nores", "o_nores", 1), ("cap_f", "o_f", NFC), ("cap_e", "o_e", NFC), ("cap_r", "o_r", NFC)):
        at = 0
        for g in got["subs"]:
            assert g[off] == at * per
            at += g[cap]
    return subs, cp


def test_capacities_floors_against_shares(harness):
    c = shares_case()
    got = run(harness, c)
    subs, cp = check_sizes(c, got, CAPS0)
    by_q = {g["Q"]: g for g in got["subs"]}
    assert by_q[103]["pairs"] == 60000 and (by_q[103]["cap_cand"], by_q[103]["cap_nores"], by_q[103]["cap_f"], by_q[103]["cap_e"], by_q[103]["cap_r"]) == (5000, 2048, 2048, 1024, 256)
    assert (by_q[5]["cap_cand"], by_q[5]["cap_nores"]) == (4096, 2048)
    assert by_q[SSV_NONE]["pairs"] == 1000 and by_q[SSV_NONE]["cap_nores"] == 1064              # every pair is recomputed exactly: pairs + 64
    assert by_q[SSV_NONE]["maxM"] == 2500
    # the workspace wish: the cells the search is expected to fill, a GB at least, the budget at most
    cells = sum(len(c.models[m]["bins"]) * (c.models[m]["fbQ"] * 64 + 64.0) * c.models[m]["fbQ"] * 64 for m in c.lane)
    assert got["cell_sum"] == cells
    assert got["ws_want"] == 1 << 30
    big = run(harness, c, caps=dict(CAPS0, ws_per_cell=400.0))
    assert big["ws_want"] == int(cells * 400.0 + 65000 * 24.0) + (256 << 20) > 1 << 30
    c.ws_budget = 64 << 20
    assert run(harness, c)["ws_want"] == 64 << 20                                                  # held to the budget
    # zone 1: 64 B per pair and 64 MB, in floats, a multiple of 32 ...
    c.ws_floats = (1 << 30) // 4
    assert run(harness, c)["z1"] == ((65000 * 64 + (64 << 20)) // 4) & ~31
    # ... and half of the workspace at the most
    c.ws_floats = (64 << 20) // 4 + 70
    z1 = run(harness, c)["z1"]
    assert z1 == (c.ws_floats // 2) & ~31 and z1 % 32 == 0 and 2 * z1 <= c.ws_floats


def test_capacities_shrunk(harness):
    """CKM_CAP_SHRINK=64: shares 64 times smaller and floors of 8"""
    c = shares_case(shrink=64)
    got = run(harness, c)
    check_sizes(c, got, CAPS0, shrink=64)
    by_q = {g["Q"]: g for g in got["subs"]}
    assert (by_q[103]["cap_cand"], by_q[103]["cap_nores"], by_q[103]["cap_f"], by_q[103]["cap_e"], by_q[103]["cap_r"]) == (60000 // (12 * 64), 60000 // (48 * 64), 8, 8, 8)
    assert by_q[5]["cap_cand"] == 8 and by_q[SSV_NONE]["cap_nores"] == 1064


def test_capacities_clamped(harness):
    c = shares_case()
    caps = dict(CAPS0, fl_cand=0xfffffff0, fl_rwork=0x80000000)
    got = run(harness, c, caps=caps)
    check_sizes(c, got, caps)
    assert all(g["cap_cand"] == CAP_MAX and g["cap_r"] == CAP_MAX for g in got["subs"])
    assert got["caps"]["rwork"] == 0xfffffff0                             # three groups of 0x7ffffff0: the shared table's own bound


def test_capacities_of_the_mixed_case(harness):
    c = mixed_case()
    check_sizes(c, run(harness, c), CAPS0)


# ---- adaptation ----------------------------------------------------------------------------------------------------------------------------------
def lesson(harness, c, caps, cnt, tops=(0, 0, 0, 0)):
    got = run(harness, c, caps=caps, cnt=[(b, k, v) for (b, k), v in cnt.items()], tops=tops)
    subs, cp = check_sizes(c, got, caps, shrink=c.shrink)
    fits, over, after = learn(subs, cp, cnt, c.shrink)
    assert got["lesson"]["fits"] == int(fits) and got["lesson"]["over"] == over
    for f in CAP_FIELDS[:19]:
        assert got["caps_after"][f] == after[f], f
    return got


def test_the_round_6_hole(harness):
    """A group of 24000 pairs wants 23994 candidates where div_cand = 12 and fl_cand = 4096 give it 4096: a floor may not grow beyond 1 << 14,
    so after one lesson the share gives the group what it asked for"""
    c = dense_case()
    first = run(harness, c)
    g = [sb["pairs"] for sb in first["subs"]].index(24000)
    assert first["subs"][g]["cap_cand"] == 4096
    got = lesson(harness, c, CAPS0, {(1 + g, CC["CAND"]): 23994})
    assert got["lesson"]["fits"] == 0 and got["lesson"]["over"] == [["cand", g, -1, 23994, 4096]]
    after = got["caps_after"]
    assert after["div_cand"] == 1 and after["fl_cand"] == 23994 + 23994 // 4 + 16            # more than the group has pairs: from the floor after all
    nxt = run(harness, c, caps=after)
    assert nxt["subs"][g]["cap_cand"] >= 23994
    # wanted fewer entries than pairs, more than a floor may hold: the divisor follows the observed share
    got = lesson(harness, c, CAPS0, {(1 + g, CC["CAND"]): 17000})
    after = got["caps_after"]
    assert after["fl_cand"] == 1 << 14 and after["div_cand"] == 24000 // (17000 + 17000 // 4 + 16) == 1
    assert run(harness, c, caps=after)["subs"][g]["cap_cand"] >= 17000


def test_a_group_that_wants_more_entries_than_it_has_pairs(harness):
    c = dense_case()
    g = [sb["pairs"] for sb in run(harness, c)["subs"]].index(12000)
    got = lesson(harness, c, CAPS0, {(1 + g, CC["EQ"] + 4): 30000})
    after = got["caps_after"]
    assert after["div_ework"] == 1 and after["fl_ework"] == 30000 + 7500 + 16
    assert run(harness, c, caps=after)["subs"][g]["cap_e"] >= 30000
    got = lesson(harness, c, CAPS0, {(1 + g, CC["EQ"] + 4): 4000000})
    assert got["caps_after"]["div_ework"] == 1 and got["caps_after"]["fl_ework"] == 1 << 20                 # the floor's last bound
    # TODAY'S ARITHMETIC, kept as it is and named in the change that moved it here: a later lesson of the same kind in the same search (another
    # class, another group) holds the floor to 1 << 14 again, so the group above is not given its 30000 entries by the next plan
    got = lesson(harness, c, CAPS0, {(1 + g, CC["EQ"] + 4): 30000, (1 + g, CC["EQ"] + 5): 1500})
    after = got["caps_after"]
    assert after["div_ework"] == 1 and after["fl_ework"] == 1 << 14
    assert run(harness, c, caps=after)["subs"][g]["cap_e"] == 1 << 14 < 30000


def test_a_kind_halves_at_most_once_per_search(harness):
    c = shares_case()
    first = run(harness, c)
    g = [sb["Q"] for sb in first["subs"]].index(103)
    assert first["subs"][g]["cap_cand"] == 5000                                                       # the share is the larger term
    got = lesson(harness, c, CAPS0, {(1 + g, CC["CAND"]): 6000, (1 + g, CC["VQ"] + 2): 7000, (1 + g, CC["VXQ"] + 14): 8000})
    assert [o[0] for o in got["lesson"]["over"]] == ["cand", "vq", "vq"]
    assert got["caps_after"]["div_cand"] == 6 and got["caps_after"]["fl_cand"] == 8000 + 2000 + 16
    assert got["lesson"]["pairs_vit"] == 7000 and got["lesson"]["pairs_vit_exact"] == 8000 and got["lesson"]["n_cand"] == 6000
    # where the floor was the larger term the divisor stays
    h = [sb["Q"] for sb in first["subs"]].index(5)
    got = lesson(harness, c, CAPS0, {(1 + h, CC["CAND"]): 5000})
    assert got["caps_after"]["div_cand"] == 12 and got["caps_after"]["fl_cand"] == 5000 + 1250 + 16


def test_one_lesson_by_hand(harness):
    """every expected value worked out by hand from the rules, none taken from the restatement: a group of 60000 pairs whose tables hold
    2048 undecided pairs, 2048 Forward items, 1024 envelopes and 256 regions (the floors: its shares are 1250, 375, 234 and 1)"""
    c = shares_case()
    exe_got = run(harness, c)
    g = [sb["Q"] for sb in exe_got["subs"]].index(103)
    cnt = {(1 + g, CC["NORES"]): 3000, (1 + g, CC["FQ"]): 2500, (1 + g, CC["BQ"]): 2600, (1 + g, CC["EQ"]): 1100, (1 + g, CC["RQ"]): 20000}
    got = run(harness, c, cnt=[(b, k, v) for (b, k), v in cnt.items()])
    assert got["lesson"] == dict(fits=0, pairs_vit=0, pairs_vit_exact=0, n_cand=0, n_nores=3000,
                                 over=[["nores", g, -1, 3000, 2048], ["fq", g, 0, 2600, 2048], ["eq", g, 0, 1100, 1024], ["rq", g, 0, 20000, 256]])
    after = got["caps_after"]
    # the floors were the larger terms: no divisor halves; a floor becomes what was asked for, a quarter more and 16
    assert (after["div_cand"], after["fl_cand"]) == (12, 4096)
    assert (after["div_nores"], after["fl_nores"]) == (48, 3000 + 750 + 16)
    assert (after["div_fwork"], after["fl_fwork"]) == (160, 2600 + 650 + 16)
    assert (after["div_ework"], after["fl_ework"]) == (256, 1100 + 275 + 16)
    # 25016 regions are more than a floor may hold: the floor stops at 1 << 14 and the divisor becomes 60000 // 25016
    assert (after["div_rwork"], after["fl_rwork"]) == (2, 1 << 14)
    assert [after[f] for f in CAP_FIELDS[:9]] == [got["caps"][f] for f in CAP_FIELDS[:9]]           # no shared table was short
    nxt = run(harness, c, caps=after)["subs"][g]
    assert (nxt["cap_cand"], nxt["cap_nores"], nxt["cap_f"], nxt["cap_e"], nxt["cap_r"]) == (5000, 3766, 3266, 1391, 30000)


def test_shrunk_tables_teach_no_floor(harness):
    c = shares_case(shrink=64)
    first = run(harness, c)
    g = [sb["Q"] for sb in first["subs"]].index(103)
    got = lesson(harness, c, CAPS0, {(1 + g, CC["CAND"]): 30000, (1 + g, CC["FQ"]): 500, (1 + g, CC["RQ"]): 100})
    after = got["caps_after"]
    assert [after[f] for f in CAP_FIELDS[14:19]] == [CAPS0[f] for f in CAP_FIELDS[14:19]]
    assert (after["div_cand"], after["div_fwork"], after["div_rwork"], after["div_nores"]) == (6, 80, 16384, 48)


def test_models_without_ssv_never_teach_div_nores(harness):
    c = shares_case()
    first = run(harness, c)
    g = [sb["Q"] for sb in first["subs"]].index(SSV_NONE)
    got = lesson(harness, c, CAPS0, {(1 + g, CC["NORES"]): 5000})
    assert got["lesson"]["over"] == [["nores", g, -1, 5000, 1064]] and got["lesson"]["fits"] == 0
    assert got["caps_after"]["div_nores"] == 48 and got["caps_after"]["fl_nores"] == 2048


def test_shared_tables_the_export_buffer_and_the_workspace_rates(harness):
    c = shares_case()
    got = lesson(harness, c, CAPS0, {(0, CC["FWORK"]): 9000, (0, CC["RWORK"]): 500, (0, CC["STATUS"]): 4 | CS_RWORK}, tops=(50000000, 0, 3000000000, 0))
    before, after = got["caps"], got["caps_after"]
    assert got["lesson"]["over"] == [["fwork", -1, -1, 9000, before["fwork"]]]
    assert after["fwork"] == 9000 + 2250 + 1024 and after["seen_rwork"] == 500 and after["hens"] == 2 * before["hens"]
    assert before["hens"] == min(before["rwork"], 8192) * (256 + 200 * 16 * 4 + 1024)
    # both zones asked for more than they had: the rates follow what was asked for, 15 % more
    z1 = got["z1"]
    assert after["z1_per_pair"] == pytest.approx(1.15 * 50000000 * 4.0 / 65000, rel=1e-6) and after["z1_per_pair"] > 64.0
    assert after["ws_per_cell"] == pytest.approx(1.15 * (3000000000 + z1) * 4.0 / got["cell_sum"], rel=1e-6) and after["ws_per_cell"] > 11.0
    # a search that fits teaches nothing
    calm = lesson(harness, c, CAPS0, {(0, CC["FWORK"]): 100, (1, CC["CAND"]): 100, (1, CC["VQ"] + 2): 90}, tops=(1000, 0, 1000, 0))
    assert calm["lesson"]["fits"] == 1 and calm["lesson"]["over"] == [] and calm["caps_after"] == calm["caps"]


def test_dense_search_reaches_a_plan_that_fits(harness):
    """plan -> counters -> lesson -> plan for the dense shape of test_queue_adaptation_reaches_a_fixed_point (tests/test_gpu_cascade.py): 36000 pairs
    in groups of 24000 and 12000, every per-group demand equal to the group's pairs.  Within the six searches the GPU test allows the plan fits, and
    it stays fitting."""
    c = dense_case()
    subs = run(harness, c)["subs"]
    assert sorted(sb["pairs"] for sb in subs) == [12000, 24000]
    cnt = {(0, CC["FWORK"]): 36000, (0, CC["EWORK"]): 36000, (0, CC["RWORK"]): 36000, (0, CC["PASS"]): 36000, (0, CC["REG"]): 72000}
    for g, sb in enumerate(subs):
        cnt[(1 + g, CC["CAND"])] = cnt[(1 + g, CC["NORES"])] = sb["pairs"]
        for k in sb["vit"]:
            cnt[(1 + g, CC["VQ"] + k)] = cnt[(1 + g, CC["VXQ"] + k)] = sb["pairs"]
        for k in sb["fb"]:
            for q in ("FQ", "BQ", "EQ", "RQ"):
                cnt[(1 + g, CC[q] + k)] = sb["pairs"]
    caps, fits = CAPS0, []
    for _search in range(6):
        got = lesson(harness, c, caps, cnt)
        fits.append(got["lesson"]["fits"])
        caps = got["caps_after"]
    took = fits.index(1) + 1 if 1 in fits else None
    print("searches until the dense shape's plan fits:", took, fits)
    assert took is not None and all(fits[took - 1:]), fits
