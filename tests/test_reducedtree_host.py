"""ReducedTree without a device: the host executor ckm_nearid_host against the plain statement of the header (tests/emu/nearid) at ==, what
ckm_nearid_check refuses, the ABI number, every golden case (tests/golden/reducedtree_cases.json, made by tools/gen_reducedtree_golden.py
from the reference's own createSmallTree.py) through the Python fallback loop and through the host executor, the order dependence of
the greedy pass, the nearly_identical.tsv resume path, the properties of `prune` on random trees against a brute-force path sum, and
GenomeTree.deduplicate read back by MarkerSetBuilder.readDuplicateSeqs."""
import itertools
import json
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.genomeTree import GenomeTree, readFasta
from checkm_amd.markerSetBuilder import MarkerSetBuilder
from checkm_amd.reducedTree import ReducedTree, limitOf, plainNearlyIdentical, prune
from checkm_amd.treeParser import read_newick, write_newick
from tests import reducedtree_synth as synth
from tests.emu import nearid as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "reducedtree_cases.json")))}

ROW_COUNTS = (1, 2, 63, 64, 65, 129, 200)
ROW_LENGTHS = (1, 7, 8, 9, 12, 13, 25, 127, 128, 129, 300)


def planted(seed, n_rows, row_len):
    """(text [n_rows, row_len] uint8, limit [n_rows] uint32) of a shape: every byte value except newline; pairs planted at exactly
    limit - 1, limit and limit + 1 differences, with the differences in the first byte, the last byte of the row and the last byte of a
    64-bit word, or spread over the whole row (several chunks: an early exit is crossed); pairs that differ only in bit 7; identical
    rows; per-row limits that differ between the rows of a tile."""
    rng = np.random.default_rng(seed)
    values = np.array([v for v in range(256) if v != 10], dtype=np.uint8)
    few = values[rng.integers(0, values.size, size=4)]
    text = np.where(rng.random((n_rows, row_len)) < 0.5, few[rng.integers(0, 4, size=(n_rows, row_len))], values[rng.integers(0, values.size, size=(n_rows, row_len))]).astype(np.uint8)
    limit = np.full(n_rows, emu.limit_of(row_len), dtype=np.uint32)
    for i in range(n_rows):                                                           # limits that differ between the rows of one tile
        if rng.random() < 0.3:
            limit[i] = rng.integers(1, row_len + 2)
    fixed = [0, row_len - 1] + [c for c in (7, 15, 127) if c < row_len]
    k = 0
    for lead in range(0, n_rows - 1, 3):
        for j in range(lead + 1, min(lead + 3, n_rows)):
            want = int(limit[lead]) + (-1, 0, 1)[k % 3]
            want = max(0, min(want, row_len))
            row = text[lead].copy()
            if k % 2 == 0:
                cols = [c for c in fixed][:want] + [int(c) for c in rng.permutation(row_len) if c not in fixed][:max(0, want - len(fixed))]
            else:
                cols = [int(c) for c in np.linspace(0, row_len - 1, num=want, dtype=np.int64)] if want else []
                cols = sorted(set(cols))
            for c in cols:
                row[c] ^= 0x80 if k % 4 < 2 or c % 2 else 0x01                  # (half of the pairs differ in bit 7 alone)
                if row[c] == 10:
                    row[c] = 11 if text[lead, c] != 11 else 12
            text[j] = row
            k += 1
    return text, limit


def shapes():
    out = [(n, 300 if n in (1, 2, 63) else (25, 129, 128, 300)[k % 4]) for k, n in enumerate(ROW_COUNTS)]
    out += [(65, L) for L in ROW_LENGTHS]
    return out


@pytest.mark.parametrize("n_rows,row_len", shapes())
def test_host_executor_equals_the_emulator(n_rows, row_len):
    text, limit = planted(n_rows * 1000 + row_len, n_rows, row_len)
    t = _lib.NearidTables(text, limit)
    want = emu.near_bits(text, limit)
    fixed, per = t.n_rows * t.row_stride + t.n_rows * 4, 64 * t.words * 8
    for budget in (1, fixed + 2 * per, 0):
        o = _lib.nearid_host(t, budget)
        assert o["near"].tolist() == want.tolist()
        assert o["nbands"] == len(emu.bands(n_rows, t.row_stride, budget if budget else 256 << 20))
        assert o["npairs"] == n_rows * (n_rows - 1) // 2


def test_planted_shapes_hold_what_they_must():
    text, limit = planted(65300, 65, 300)
    d = emu.diffs(text)
    margins = set()
    for i in range(65):
        for j in range(i + 1, 65):
            if abs(int(d[i, j]) - int(limit[i])) <= 1:
                margins.add(int(d[i, j]) - int(limit[i]))
    assert margins == {-1, 0, 1}
    assert len(set(limit[:64].tolist())) > 3 and set(np.unique(text).tolist()) >= set(range(0x80, 0x100)) and 10 not in text
    pairs7 = [(i, j) for i in range(65) for j in range(i + 1, min(i + 3, 65)) if d[i, j] and ((text[i] ^ text[j]) & 0x7F).max() == 0]
    assert pairs7                                                                     # pairs that differ in bit 7 alone
    near = emu.near_bits(text, limit)
    assert near.any() and not near.all()


def test_every_byte_value_counts_as_itself():
    base = np.arange(256, dtype=np.uint8)
    text = np.stack([base, base ^ 0x80, base ^ 0x01, base, np.zeros(256, dtype=np.uint8)])
    # differences: rows 0-1, 0-2, 1-2, 1-3, 2-3: all 256 columns; 0-3: none; 0-4: 255 (both hold 0 in column 0); 1-4: 255 (column 0x80)
    o = _lib.nearid_host(_lib.NearidTables(text, [257, 256, 1, 1, 1]))
    assert o["near"][:, 0].tolist() == [0b11110, 0b10000, 0, 0, 0] == emu.near_bits(text, [257, 256, 1, 1, 1])[:, 0].tolist()
    o = _lib.nearid_host(_lib.NearidTables(text, [256, 257, 1, 1, 1]))
    assert o["near"][:, 0].tolist() == [0b11000, 0b11100, 0, 0, 0] == emu.near_bits(text, [256, 257, 1, 1, 1])[:, 0].tolist()


def test_refusals_of_the_check():
    text = np.zeros((4, 32), dtype=np.uint8)
    limit = np.ones(4, dtype=np.uint32)

    def code(n_rows=4, row_len=20, row_stride=32, limit=limit, text=text):
        a = _lib.NearidArgs(text.ctypes.data if text is not None else None, n_rows, row_len, row_stride, limit.ctypes.data if limit is not None else None)
        return _lib.load().ckm_nearid_check(_lib.C.byref(a))

    assert code() == 0 and code(row_len=32) == 0
    assert code(n_rows=0) == -1 and code(row_len=0) == -1 and code(text=None) == -1 and code(limit=None) == -1
    assert code(limit=np.array([1, 1, 0, 1], dtype=np.uint32)) == -1
    assert code(row_len=33) == -1 and code(row_stride=24) == -1 and code(row_len=8, row_stride=8) == -1
    # sizes beyond the header's limits are refused before anything is read (the arrays here are far smaller)
    assert code(n_rows=(1 << 17) + 1, row_len=1, row_stride=16) == -7
    assert code(n_rows=1, row_len=1, row_stride=(1 << 24) + 16) == -7
    assert code(n_rows=1 << 17, row_len=1, row_stride=1 << 24) == -7
    for kw in (dict(n_rows=0), dict(row_len=0), dict(row_stride=24)):
        assert emu.refusal(True, kw.get("n_rows", 4), kw.get("row_len", 20), kw.get("row_stride", 32), limit) == "EINVAL"
    assert emu.refusal(True, (1 << 17) + 1, 1, 16, None) == "EINVAL" and emu.refusal(True, (1 << 17) + 1, 1, 16, []) == "ERANGE"
    with pytest.raises(_lib.CkmError):
        _lib.nearid_check(_lib.NearidTables(text[:, :20], [1, 1, 0, 1]))
    assert _lib.NEARID_MAX_ROWS == emu.MAX_ROWS and _lib.NEARID_MAX_STRIDE == emu.MAX_STRIDE and _lib.NEARID_MAX_TEXT_BYTES == emu.MAX_TEXT_BYTES


def test_abi_number_and_exports():
    L = _lib.load()
    assert L.ckm_abi_version() == 12
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    assert "#define CKM_ABI_VERSION 12 " in header and "ckm_nearid_*" in header.split("#define CKM_ABI_VERSION 12")[1].split("\n")[0]
    for name in ("ckm_nearid_check", "ckm_nearid_host", "ckm_nearid_run"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_limits_follow_the_reference_expression():
    assert [limitOf("x" * n) for n in (1, 12, 13, 24, 25, 37, 38, 100, 6988)] == [1, 1, 1, 1, 2, 2, 3, 8, 559]
    assert [emu.limit_of(n) for n in (12, 13, 25, 6988)] == [1, 1, 2, 559]
    a = "ACDEFGHIKLMNP" * 2
    assert plainNearlyIdentical(a[:12], a[:12]) and not plainNearlyIdentical(a[:12], a[:11] + "-")
    assert plainNearlyIdentical(a[:25], a[:24] + "-") and not plainNearlyIdentical(a[:25], a[:23] + "--")


def refusing_runner(tables, budget_bytes=0):
    raise _lib.CkmError(-7, "refused for the test")


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_clusters(name):
    c = CASES[name]
    rows = {k: s for k, s in c["rows"]}
    equal = len(set(len(s) for s in rows.values())) == 1 and all(rows.values())
    for runner, fallbacks in ((_lib.nearid_host, 0 if equal else 1), (refusing_runner, 1)):
        r = ReducedTree(runner=runner)
        got = r.nearlyIdentical(rows)
        assert [sorted(x) for x in got] == c["clusters"], runner.__name__
        assert r.lastInfo["python_fallbacks"] == fallbacks and r.lastInfo["rows"] == len(rows)
        order = {k: n for n, k in enumerate(rows)}
        assert all(x == sorted(x, key=order.get) for x in got)                         # members in file order
    assert sorted(map(tuple, c["tsv"])) == sorted(map(tuple, c["clusters"]))


def test_goldens_cover_what_they_must():
    assert {len(r[1]) for r in CASES["columns_12"]["rows"]} == {12} and CASES["columns_12"]["clusters"][0] == ["a", "c"]
    assert CASES["columns_13"]["clusters"][0] == ["a", "c"] and CASES["columns_25"]["clusters"][0] == ["a", "b", "c", "f"]
    assert CASES["columns_100"]["clusters"][0] == ["ends", "lead", "same", "seven"]
    assert CASES["chain_abc"]["clusters"] == [["a", "b"], ["c"]] and CASES["chain_bac"]["clusters"] == [["a", "b", "c"]]
    assert ["bit7"] in CASES["raw_bytes"]["clusters"] and ["lower"] in CASES["raw_bytes"]["clusters"]
    assert len(set(len(r[1]) for r in CASES["unequal_lengths"]["rows"])) > 2 and len(CASES["seventy_rows"]["rows"]) == 70


def test_the_greedy_order_is_not_transitive():
    rnd = random.Random(5)
    a = "".join(rnd.choice("ACDEFGHIKL") for _ in range(100))
    flip = lambda s, cols: "".join(("-" if k in cols else ch) for k, ch in enumerate(s))
    b = flip(a, range(0, 5))
    c = flip(b, range(50, 55))
    assert plainNearlyIdentical(a, b) and plainNearlyIdentical(b, c) and not plainNearlyIdentical(a, c)
    for runner in (_lib.nearid_host, refusing_runner):
        r = ReducedTree(runner=runner)
        assert r.nearlyIdentical({"a": a, "b": b, "c": c}) == [["a", "b"], ["c"]]
        assert r.nearlyIdentical({"b": b, "a": a, "c": c}) == [["b", "a", "c"]]
        assert r.nearlyIdentical({"c": c, "a": a, "b": b}) == [["c", "b"], ["a"]]


def test_resume_from_nearly_identical_tsv(tmp_path, capsys):
    def never(tables, budget_bytes=0):
        raise AssertionError("the rows were compared")
    rows = {k: s for k, s in CASES["columns_100"]["rows"]}
    fresh = ReducedTree(runner=_lib.nearid_host).nearlyIdenticalGenomes(rows, str(tmp_path))
    text = open(tmp_path / "nearly_identical.tsv").read()
    assert text == "".join("\t".join(x) + "\n" for x in fresh) and [sorted(x) for x in fresh] == CASES["columns_100"]["clusters"]
    assert "Number of dereplicated taxa: %d" % len(fresh) in capsys.readouterr().out
    assert ReducedTree(runner=never).nearlyIdenticalGenomes(rows, str(tmp_path)) == fresh
    open(tmp_path / "nearly_identical.tsv", "w").write("x\ty \nz\n")
    assert ReducedTree(runner=never).nearlyIdenticalGenomes(rows, str(tmp_path)) == [["x", "y"], ["z"]]
    assert "Number of taxa: 3" in capsys.readouterr().out


# ---- prune ------------------------------------------------------------------------------------------------------------------------------------
def random_newick(rnd, nleaves):
    nodes = ["L%d:%r" % (k, round(rnd.random(), 3)) for k in range(nleaves)]
    label = 0
    while len(nodes) > 1:
        k = min(len(nodes), rnd.choice((2, 2, 2, 3, 4)))
        picked = [nodes.pop(rnd.randrange(len(nodes))) for _ in range(k)]
        label += 1
        nodes.append("(" + ",".join(picked) + ")N%d:%r" % (label, round(rnd.random(), 3)))
    return nodes[0].rsplit(":", 1)[0] + ";"


def nodes_of(tree):
    out, stack = [], [tree.root]
    while stack:
        v = stack.pop()
        out.append(v)
        stack.extend(v.children)
    return out


def path_sums(tree):
    """{(leaf a, leaf b): (path length by brute force, label of the common ancestor)}"""
    def chain(v):
        out = []
        while v is not None:
            out.append(v)
            v = v.parent
        return out
    leaves = list(tree.root.leaves())
    out = {}
    for a, b in itertools.combinations(leaves, 2):
        ca, cb = chain(a), chain(b)
        common = next(x for x in ca if any(x is y for y in cb))
        length = sum(x.length for x in ca[:ca.index(common)]) + sum(x.length for x in cb[:[id(y) for y in cb].index(id(common))])
        out[(a.taxon, b.taxon)] = (length, common.label)
    return out


@pytest.mark.parametrize("seed", range(12))
def test_prune_properties_on_random_trees(seed):
    rnd = random.Random(seed)
    nleaves = rnd.randint(4, 40)
    text = random_newick(rnd, nleaves)
    before = path_sums(read_newick(text))
    keep = set(rnd.sample(["L%d" % k for k in range(nleaves)], rnd.randint(2, nleaves)))
    pruned = prune(read_newick(text), keep | {"absent"})
    assert set(leaf.taxon for leaf in pruned.root.leaves()) == keep
    assert pruned.root.parent is None and all(len(v.children) >= 2 for v in nodes_of(pruned) if v.children)
    assert all(c.parent is v for v in nodes_of(pruned) for c in v.children)
    after = path_sums(pruned)
    assert len(after) == len(keep) * (len(keep) - 1) // 2
    surviving = set(v.label for v in nodes_of(pruned) if v.children)
    assert surviving <= set(v.label for v in nodes_of(read_newick(text)) if v.children)     # labels of surviving nodes are unchanged
    for (a, b), (length, label) in after.items():
        was = before[(a, b)] if (a, b) in before else before[(b, a)]
        assert label == was[1]                                                        # the common ancestor of a kept pair survives, label unchanged
        assert abs(length - was[0]) <= 1e-12 * max(1.0, was[0])                      # the same lengths summed in another grouping
    again = read_newick(write_newick(pruned))
    assert path_sums(again).keys() == after.keys()


def test_prune_by_hand():
    t = prune(read_newick("(((a:1,b:2)x:3,c:4)y:5,(d:6,(e:7,f:8)z:9)w:10)r;"), ["a", "c", "e"])
    assert write_newick(t) == "((a:4.0,c:4.0)y:5.0,e:26.0)r;"
    t = prune(read_newick("(((a:1,b:2)x:3,c:4)y:5,(d:6,(e:7,f:8)z:9)w:10)r;"), ["a", "b"])
    assert write_newick(t) == "(a:1.0,b:2.0)x;" and t.find_leaf("a") is not None and t.find_leaf("c") is None
    assert write_newick(prune(read_newick("((a:1,b:2)x:3,c:4)r;"), ["a", "b", "c"]), labels=False) == "((a:1.0,b:2.0):3.0,c:4.0);"
    with pytest.raises(ValueError):
        prune(read_newick("((a:1,b:2)x:3,c:4)r;"), ["q"])


# ---- deduplicate ------------------------------------------------------------------------------------------------------------------------------
def test_deduplicate_round_trips_through_readDuplicateSeqs(tmp_path):
    rows = [("IMG_1", "ACD-"), ("IMG_2", "ACDE"), ("IMG_3", "ACD-"), ("g4", "acd-"), ("IMG_5", "ACDE"), ("IMG_6", "ACD-"), ("IMG_7", "WWWW")]
    src = tmp_path / "genome_tree.concatenated.fasta"
    open(src, "w").write("".join(">%s\n%s\n" % r for r in rows))
    derep, dups = str(tmp_path / "derep.fasta"), str(tmp_path / "genome_tree.derep.txt")
    got = GenomeTree.deduplicate(str(src), derep, dups)
    assert got == {"IMG_1": ["IMG_3", "IMG_6"], "IMG_2": ["IMG_5"]}
    assert list(readFasta(derep).items()) == [("IMG_1", "ACD-"), ("IMG_2", "ACDE"), ("g4", "acd-"), ("IMG_7", "WWWW")]
    assert open(dups).read() == "IMG_1 IMG_3 IMG_6\nIMG_2 IMG_5\n"
    assert MarkerSetBuilder(None).readDuplicateSeqs(dups) == got
