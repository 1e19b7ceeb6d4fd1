"""GenomeTree without a device: the host part against the goldens of the reference's scripts, and the host executor of gtree_dev.h
(tests/emu/genometree.py, and ckm_gtree_host of the library) against a second formulation -- a plain numpy neighbour joining that
recomputes every R from scratch --, against additive matrices, against sequences evolved down a known tree, and against math.log."""
import json
import math
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.genomeTree import GenomeTree
from checkm_amd.img import IMG
from checkm_amd.pplacer import nodes_of, parse_newick, plain_name
from tests.emu import genometree as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "genometree_cases.json")
AA = "ARNDCQEGHILKMFPSTWYV"
LOG_BOUND = 2 * 4.4e-16          # twice the largest relative difference from math.log measured over the arguments below


def host_tree():
    return GenomeTree(runner=emu.runner)


# ---- trees as sets of splits ---------------------------------------------------------------------------------------------------------------
def canon(mask, n):
    return ((1 << n) - 1) ^ mask if mask & 1 else mask


def edges_of_text(text, ids):
    """canonical split -> length of its edge, the two edges at a root of two children taken as one; trivial splits included"""
    root = parse_newick(text)
    n = len(ids)
    clade = GenomeTree._clades(root, {name: k for k, name in enumerate(ids)})
    out = {}
    for v in nodes_of(root):
        if v.parent is None:
            continue
        key = canon(clade[v], n)
        out[key] = out.get(key, 0.0) + float(v.length)
    return out


def inner(edges, n):
    return set(k for k in edges if 1 < bin(k).count("1") < n - 1)


def plain_nj(D):
    """Saitou-Nei with the Studier-Keppler criterion, every R summed afresh each round; canonical split -> length."""
    D = np.array(D, dtype=np.float64)
    n0 = D.shape[0]
    clade = [1 << k for k in range(n0)]
    act = list(range(n0))
    edges = {}

    def put(mask, length):
        key = canon(mask, n0)
        edges[key] = edges.get(key, 0.0) + max(length, 0.0)

    while len(act) > 3:
        n = len(act)
        sub = D[np.ix_(act, act)]
        R = sub.sum(axis=1) - np.diag(sub)
        Q = (n - 2) * sub - R[:, None] - R[None, :]
        Q[np.tril_indices(n)] = np.inf
        a, b = np.unravel_index(np.argmin(Q), Q.shape)
        i, j = act[a], act[b]
        d = D[i, j]
        li = d / 2 + (R[a] - R[b]) / (2 * (n - 2))
        lj = d - li
        if li < 0:
            li, lj = 0.0, d
        elif lj < 0:
            li, lj = d, 0.0
        put(clade[i], li)
        put(clade[j], lj)
        new = (D[i] + D[j] - d) / 2
        D[i, :] = new
        D[:, i] = new
        D[i, i] = 0.0
        clade[i] |= clade[j]
        act.pop(b)
    if len(act) == 3:
        x, y, z = act
        put(clade[x], (D[x, y] + D[x, z] - D[y, z]) / 2)
        put(clade[y], (D[x, y] + D[y, z] - D[x, z]) / 2)
        put(clade[z], (D[x, z] + D[y, z] - D[x, y]) / 2)
    else:
        put(clade[act[0]], D[act[0], act[1]])
    return edges


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def random_tree(rng, n, lo=0.05, hi=0.25):
    """A random unrooted binary tree over n leaves as (parent list, length list) of a rooted form whose root has three children; nodes
    0 .. n-1 are the leaves."""
    tops = list(range(n))
    parent, length = {}, {}
    nxt = n
    while len(tops) > 3:
        a, b = rng.sample(range(len(tops)), 2)
        x, y = tops[a], tops[b]
        for v in (x, y):
            parent[v], length[v] = nxt, rng.uniform(lo, hi)
        tops = [t for k, t in enumerate(tops) if k not in (a, b)] + [nxt]
        nxt += 1
    for v in tops:
        parent[v], length[v] = nxt, rng.uniform(lo, hi)
    return parent, length, nxt


def tree_edges(parent, length, root, n):
    clade = {k: 1 << k for k in range(n)}
    for v in sorted(parent):
        clade[parent[v]] = clade.get(parent[v], 0) | clade[v]
    return {canon(clade[v], n): length[v] for v in parent}


def path_matrix(parent, length, root, n):
    def up(v):
        out, d = {}, 0.0
        while v != root:
            d += length[v]
            v = parent[v]
            out[v] = d
        return out

    ups = [up(k) for k in range(n)]
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = min(ups[i][v] + ups[j][v] for v in ups[i] if v in ups[j])
    return D


def evolved_case(seed=5, n=16, ncols=2000, gaps=0.10):
    """Sequences evolved down a random tree under the equal-rates 20-state model; 10 % of the cells are gaps.  Returns (ids, seqs, the
    tree's canonical split -> length)."""
    rng = random.Random(seed)
    parent, length, root = random_tree(rng, n)
    npr = np.random.RandomState(seed)
    children = {}
    for v, p in parent.items():
        children.setdefault(p, []).append(v)
    state = {root: npr.randint(0, 20, ncols)}
    stack = [root]
    while stack:
        p = stack.pop()
        for c in children.get(p, ()):
            change = npr.random_sample(ncols) < (19.0 / 20.0) * (1.0 - math.exp(-20.0 / 19.0 * length[c]))
            other = (state[p] + npr.randint(1, 20, ncols)) % 20
            state[c] = np.where(change, other, state[p])
            stack.append(c)
    letters = np.frombuffer(AA.encode(), dtype=np.uint8)
    ids = ["g%02d" % k for k in range(n)]
    seqs = {}
    for k in range(n):
        row = letters[state[k]].copy()
        row[npr.random_sample(ncols) < gaps] = ord("-")
        seqs[ids[k]] = row.tobytes().decode()
    return ids, seqs, tree_edges(parent, length, root, n)


def plain_distances(seqs, ids, model):
    rows = np.array([np.frombuffer(seqs[k].encode(), dtype=np.uint8) for k in ids])
    known = rows != ord("-")
    n = len(ids)
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            both = known[i] & known[j]
            p = float(((rows[i] != rows[j]) & both).sum()) / both.sum()
            D[i, j] = 0.0 if i == j else -math.log(1 - p) if model == "poisson" else -math.log(1 - p - 0.2 * p * p)
    return D


@pytest.fixture(scope="module")
def evolved():
    return evolved_case()


# ---- goldens -------------------------------------------------------------------------------------------------------------------------------
def test_concatenate_and_bootstrap_columns_match_the_goldens(tmp_path):
    cases = json.load(open(GOLDEN))
    for case in cases["concatenate"]:
        d = tmp_path / case["name"]
        for rel, text in case["files"].items():
            p = d / rel
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(text)
        img = IMG(str(d / "img_metadata.tsv"), str(d / "tigrfam2pfam.tsv"), str(d / "genomes"))
        out_aln, out_tax = str(d / "out.faa"), str(d / "out.tax")
        GenomeTree().concatenate(str(d / "gene_trees"), str(d / "alignments"), case["extension"], out_aln, out_tax, img)
        got_aln, got_tax = open(out_aln).read(), open(out_tax).read()
        assert got_tax == case["taxonomy"]
        if case["order_free"]:
            assert got_aln == case["alignment"]
        else:                          # the reference wrote its records in the order of a dict of its Python: the same records, any order
            records = lambda t: sorted(t.split(">")[1:])
            assert records(got_aln) == records(case["alignment"])
            if case["name"] == "five_genomes":                        # file order: first appearance over the sorted alignment files
                assert [r.split("\n")[0] for r in got_aln.split(">")[1:]] == ["IMG_64000000%d" % k for k in (1, 2, 3, 4, 5)]
    for case in cases["bootstrap"]:
        random.seed(case["seed"])
        cols = GenomeTree.bootstrapColumns(case["alignmentLen"], case["numBootstraps"])
        assert cols.dtype == np.uint32 and cols.tolist() == case["cols"]


# ---- the executor against a second formulation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 17, 64])
def test_executor_against_plain_neighbour_joining(n):
    """Random matrices without ties: the path lengths of a random tree, every entry moved by up to 1 %.  (Matrices far from any tree give
    negative raw lengths, and which sibling then takes the whole distance depends on which of two complementary pairs -- equal in Q but
    for rounding -- is joined: the rule has its own test below.)"""
    rng = np.random.RandomState(100 + n)
    for rep in range(3):
        parent, length, root = random_tree(random.Random(1000 * n + rep), n)
        D = path_matrix(parent, length, root, n) * rng.uniform(0.99, 1.01, (n, n))
        D = np.triu(D, 1) + np.triu(D, 1).T
        ids = ["t%d" % k for k in range(n)]
        got = edges_of_text(host_tree().neighbourJoin(ids, D), ids)
        want = plain_nj(D)
        assert set(got) == set(want)
        for k in want:
            print(n, rep, k, got[k], want[k])
            assert abs(got[k] - want[k]) <= 1e-9


def test_additive_matrix_returns_the_tree():
    n = 33
    parent, length, root = random_tree(random.Random(33), n)
    D = path_matrix(parent, length, root, n)
    ids = ["a%d" % k for k in range(n)]
    want = tree_edges(parent, length, root, n)
    got = edges_of_text(host_tree().neighbourJoin(ids, D), ids)
    assert set(got) == set(want)
    assert max(abs(got[k] - want[k]) for k in want) <= 1e-9


def test_recovery_of_an_evolved_tree(evolved):
    ids, seqs, truth = evolved
    n = len(ids)
    assert inner(plain_nj(plain_distances(seqs, ids, "poisson")), n) == inner(truth, n)          # the fixture itself, by the plain formulation first
    got = edges_of_text(host_tree().infer(seqs, model="poisson"), ids)
    assert inner(got, n) == inner(truth, n)


def test_fixture_supports_of_the_true_splits(evolved):
    """What the device's end-to-end test relies on: every true split of the fixture carries a support above 0.5."""
    ids, seqs, truth = evolved
    gt = host_tree()
    random.seed(11)
    text = gt.bootstrap(seqs, gt.infer(seqs, model="poisson"), numBootstraps=20, model="poisson")
    root = parse_newick(text)
    clade = GenomeTree._clades(root, {name: k for k, name in enumerate(ids)})
    seen = {}
    for v in nodes_of(root):
        if v.children and v.parent is not None:
            seen[canon(clade[v], len(ids))] = float(v.name)
            assert v.name == "%.3f" % float(v.name)
    assert set(seen) == inner(truth, len(ids)) and min(seen.values()) > 0.5
    # the text loads unchanged in treeParser.Tree: every leaf is found, the supports are the labels of the internal nodes
    from checkm_amd.treeParser import read_newick
    tree = read_newick(text)
    assert all(tree.find_leaf(name) is not None for name in ids) and len(list(tree.root.leaves())) == len(ids)


# ---- the logarithm ---------------------------------------------------------------------------------------------------------------------------
def test_header_log_against_math_log():
    ps = sorted(set(d / float(c) for c in range(1, 513) for d in range(0, c + 1)))
    args = set()
    for p in ps:
        for model in (0, 1):
            a = emu.arg(p, model)
            assert a == ((1.0 - p) - 0.2 * (p * p) if model == 0 else 1.0 - p)
            if a > 0.0:
                args.add(a)
    xs = np.array(sorted(args | set(p for p in ps if p > 0.0)))
    got = emu.logs(xs)
    worst = 0.0
    for x, y in zip(xs.tolist(), got.tolist()):
        ref = math.log(x)
        assert (y == 0.0) if ref == 0.0 else True
        if ref != 0.0:
            worst = max(worst, abs(y - ref) / abs(ref))
    print("arguments %d, largest relative difference %.3e" % (len(xs), worst))
    assert LOG_BOUND < 1e-12 and worst <= LOG_BOUND
    for x in (2.0, 10.0, 1e-300, 1e300, 0.75, 1.5):
        assert abs(emu.log(x) - math.log(x)) <= LOG_BOUND * abs(math.log(x))


def test_library_host_executor_gives_the_emulator_bits(evolved):
    """ckm_gtree_host (the library's build of the header) and the g++ build agree on every count, distance bit and merge row."""
    ids, seqs, _ = evolved
    random.seed(3)
    cols = GenomeTree.bootstrapColumns(2000, 2)
    for model in ("kimura", "poisson", "p"):
        _, t = GenomeTree()._tables(seqs, cols=cols, model=model)
        a, b = _lib.gtree_host(t, counts=True, dist=True), emu.gtree_run(None, t, counts=True, dist=True)
        for f in ("compared", "differ", "merge_ij"):
            assert np.array_equal(a[f], b[f])
        for f in ("dist", "merge_len"):
            assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64))


# ---- small cases -----------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_pair():
    D = np.ones((6, 6)) - np.eye(6)
    r = emu.gtree_run(None, _lib.GtreeTables(matrices=D[None]))
    assert r["merge_ij"][0].tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [0, 5]]
    assert r["merge_len"][0].tolist() == [[0.5, 0.5], [0.0, 0.5], [0.0, 0.5], [0.0, 0.5], [0.25, 0.25]]


def test_identical_rows_gap_rows_and_max_dist():
    seqs = {"a": "ACDEFGHIKL", "b": "ACDEFGHIKL", "c": "ACDEFGHIKV", "gaps": "-.X*BZ~ ?-", "d": "acdeyyyyyy"}
    gt = host_tree()
    ids, cmp_, dif = gt.pairCounts(seqs)
    assert cmp_.tolist() == [[10, 10, 10, 0, 10], [10, 10, 10, 0, 10], [10, 10, 10, 0, 10], [0, 0, 0, 0, 0], [10, 10, 10, 0, 10]]
    assert dif[0].tolist() == [0, 0, 1, 0, 6] and dif[2].tolist() == [1, 1, 0, 0, 6] and np.array_equal(dif, dif.T)
    _, D = gt.distances(seqs, model="kimura", maxDist=3.0)
    assert D[0, 1] == 0.0 and not np.signbit(D[0, 1]) and D[0, 3] == 3.0 and D[3, 4] == 3.0 and np.array_equal(D, D.T) and not D.diagonal().any()
    assert D[0, 2] == -emu.log((1.0 - 0.1) - 0.2 * (0.1 * 0.1)) and abs(D[0, 2] - -math.log(1 - 0.1 - 0.2 * 0.01)) < 1e-15
    _, P = gt.distances(seqs, model="p")
    assert P[0, 4] == 0.6 and P[0, 3] == 3.0
    _, small = gt.distances(seqs, model="poisson", maxDist=0.5)
    assert small[0, 4] == 0.5 and small[0, 3] == 0.5 and small[0, 2] == -emu.log(0.9)
    # a pair that differs everywhere: the argument of the logarithm is not positive
    _, far = gt.distances({"x": "AAAA", "y": "CCCC"}, model="poisson", maxDist=7.0)
    assert far[0, 1] == 7.0
    text = gt.infer(seqs)
    e = edges_of_text(text, ids)
    assert e[canon(1 << 0, 5)] == 0.0 and e[canon(1 << 1, 5)] == 0.0          # the identical rows sit on edges of length 0
    assert sorted(plain_name(v.name) for v in nodes_of(parse_newick(text)) if not v.children) == sorted(ids)
    assert len(parse_newick(text).children) == 2


def test_negative_length_rule():
    # d(0,1) is small but row 0 is far from everything else: the raw length of 1's edge is negative
    D = np.array([[0, 0.1, 1.0, 1.0, 1.0], [0.1, 0, 0.3, 0.3, 0.3], [1.0, 0.3, 0, 0.5, 0.5], [1.0, 0.3, 0.5, 0, 0.5], [1.0, 0.3, 0.5, 0.5, 0]])
    r = emu.gtree_run(None, _lib.GtreeTables(matrices=D[None]))
    rows = {tuple(ij): tuple(ln) for ij, ln in zip(r["merge_ij"][0].tolist(), r["merge_len"][0].tolist())}
    assert rows[(0, 1)] == (0.1, 0.0)
    assert (r["merge_len"] >= 0.0).all()


def test_two_and_three_rows():
    gt = host_tree()
    assert gt.neighbourJoin(["a", "b"], [[0, 0.5], [0.5, 0]]) == "(a:0.25,b:0.25);"
    assert gt.neighbourJoin(["a", "b", "c"], [[0, 0.3, 0.5], [0.3, 0, 0.6], [0.5, 0.6, 0]]) == "((a:%r,b:%r):%r,c:%r);" % (
        ((0.3 + 0.5) - 0.6) * 0.5, ((0.3 + 0.6) - 0.5) * 0.5, ((0.5 + 0.6) - 0.3) * 0.5 * 0.5, ((0.5 + 0.6) - 0.3) * 0.5 * 0.5)


def test_batches_change_nothing(evolved):
    ids, seqs, _ = evolved
    random.seed(9)
    cols = GenomeTree.bootstrapColumns(2000, 5)
    _, t = GenomeTree()._tables(seqs, cols=cols, model="poisson")
    per_tree = 16 * 2000 + 16 * 16 * 16 + 16 * 64
    runs = [emu.gtree_run(None, t, budget_bytes=b) for b in (1, per_tree * 2, per_tree * 100)]
    assert [r["nrounds"] for r in runs] == [6, 3, 1]
    for r in runs[1:]:
        assert np.array_equal(r["merge_ij"], runs[0]["merge_ij"]) and np.array_equal(r["merge_len"].view(np.uint64), runs[0]["merge_len"].view(np.uint64))
    # a replicate that draws every column in order is the alignment's own tree
    _, same = GenomeTree()._tables(seqs, cols=np.arange(2000)[None], model="poisson")
    r = emu.gtree_run(None, same)
    assert np.array_equal(r["merge_ij"][0], r["merge_ij"][1]) and np.array_equal(r["merge_len"][0], r["merge_len"][1])


def test_exact_supports_on_hand_made_replicates():
    ids = ["a", "b", "c", "d", "e"]
    tree = "((a:1,b:1):1,(c:1,(d:1,e:1):1):1);"
    m = lambda pairs: GenomeTree._splits_of_merges(5, np.array(pairs, dtype=np.uint32))
    ab_de = m([[0, 1], [3, 4], [2, 3], [0, 2]])          # ((a,b),(c,(d,e)))
    ab_cd = m([[0, 1], [2, 3], [2, 4], [0, 2]])          # ((a,b),((c,d),e))
    ac_de = m([[0, 2], [3, 4], [1, 3], [0, 1]])          # ((a,c),(b,(d,e)))
    assert GenomeTree.supportTree(tree, ids, [ab_de, ab_cd, ac_de, ab_de]) == "((a:1,b:1)0.750:1,(c:1,(d:1,e:1)0.750:1)0.750:1);"
    assert GenomeTree.supportTree(tree, ids, [ac_de, ab_cd, ab_cd]) == "((a:1,b:1)0.667:1,(c:1,(d:1,e:1)0.333:1)0.667:1);"
    assert GenomeTree.supportTree(tree, ids, []) == "((a:1,b:1)0.000:1,(c:1,(d:1,e:1)0.000:1)0.000:1);"
    with pytest.raises(ValueError):
        GenomeTree.supportTree("((a:1,b:1):1,(c:1,(d:1,x:1):1):1);", ids, [ab_de])


def test_reroot_branches():
    tree = "((a:1,b:2)0.9:1,c:3,(d:1,(e:1,f:2)0.7:1)0.8:4);"
    # the outgroup is one side of an edge: the root splits that edge in half, the support stays with the edge
    assert GenomeTree.reroot(tree, ["e", "f", "d"]) == "((d:1.0,(e:1.0,f:2.0)0.7:1.0)0.8:2.0,((a:1.0,b:2.0)0.9:1.0,c:3.0)0.8:2.0);"
    assert GenomeTree.reroot(tree, ["c"]) == "(c:1.5,((a:1.0,b:2.0)0.9:1.0,(d:1.0,(e:1.0,f:2.0)0.7:1.0)0.8:4.0):1.5);"
    # the complement side counts as well: {a, b, c} is what the edge above (d, (e, f)) leaves
    assert GenomeTree.reroot(tree, ["a", "b", "c"]) == "(((a:1.0,b:2.0)0.9:1.0,c:3.0)0.8:2.0,(d:1.0,(e:1.0,f:2.0)0.7:1.0)0.8:2.0);"
    # not monophyletic, empty, all leaves: the midpoint of the longest path, b .. f: 2 + 1 + 4 + 1 + 2 = 10
    mid = "(((a:1.0,b:2.0)0.9:1.0,c:3.0)0.8:2.0,(d:1.0,(e:1.0,f:2.0)0.7:1.0)0.8:2.0);"          # (the side of the path's first leaf, b, first)
    for group in (["a", "d"], [], ["a", "b", "c", "d", "e", "f"], ["nobody"]):
        assert GenomeTree.reroot(tree, group) == mid
    # a root of two children is dissolved first; ties go to the first pair of leaves as written
    assert GenomeTree.reroot("((a:1,b:1):0.5,(c:1,d:1):0.5);", []) == "((a:1.0,b:1.0):0.5,(c:1.0,d:1.0):0.5);"
    assert GenomeTree.reroot("(a:1,b:3);", []) == "(a:2.0,b:2.0);"
    root = GenomeTree.reroot(parse_newick(tree), ["c"])
    assert [plain_name(v.name) for v in nodes_of(root) if not v.children] == ["c", "a", "b", "d", "e", "f"] and len(root.children) == 2
    # a dendropy-free check of the rule on the evolved fixture's shape: the longest path's halves are equal
    far = lambda v: 0.0 if not v.children else max(float(c.length) + far(c) for c in v.children)
    mid_root = GenomeTree.reroot(parse_newick(tree), [])
    assert abs((float(mid_root.children[0].length) + far(mid_root.children[0])) - (float(mid_root.children[1].length) + far(mid_root.children[1]))) < 1e-12


def test_reroot_keeps_the_tree(evolved):
    """On the fixture's tree: the leaves, the total length and the inner splits stay; a true clade as outgroup becomes a child of the root."""
    ids, seqs, truth = evolved
    n = len(ids)
    text = host_tree().infer(seqs, model="poisson")
    total = lambda t: sum(float(v.length) for v in nodes_of(parse_newick(t)) if v.parent is not None)
    group = max((k for k in inner(truth, n)), key=lambda k: bin(k).count("1"))
    names = [ids[b] for b in range(n) if group >> b & 1]
    for outgroup in (names, []):
        rooted = GenomeTree.reroot(text, outgroup)
        assert inner(edges_of_text(rooted, ids), n) == inner(truth, n) and abs(total(rooted) - total(text)) < 1e-12
        root = parse_newick(rooted)
        assert len(root.children) == 2
        if outgroup:
            clade = GenomeTree._clades(root, {name: k for k, name in enumerate(ids)})
            assert clade[root.children[0]] == group and root.children[0].length == root.children[1].length


# ---- refusals, ABI ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    gt = host_tree()
    N, L = _lib.GTREE_MAX_ROWS, _lib.GTREE_MAX_COLS
    with pytest.raises(ValueError, match=str(N)):
        gt.infer({"r%d" % k: "A" for k in range(N + 1)})
    with pytest.raises(ValueError, match=str(L)):
        gt.infer({"a": "A" * (L + 1), "b": "C" * (L + 1)})
    with pytest.raises(ValueError, match="ASCII"):
        gt.infer({"a": "ACé", "b": "ACD"})
    with pytest.raises(ValueError):
        gt.infer({"a": "ACD", "b": "AC"})
    with pytest.raises(ValueError):
        gt.infer({"a": "ACD"})
    with pytest.raises(ValueError):
        gt.infer({"a": "ACD", "b": "ACD"}, model="wag")
    with pytest.raises(ValueError):
        gt.neighbourJoin(["a", "b", "c"], [[0, 1, 2], [1, 0, 3], [2, 4, 0]])
    with pytest.raises(ValueError):
        gt.neighbourJoin(["a", "b"], [[0, float("nan")], [float("nan"), 0]])
    # the library's own check, on the arguments as the device entry would get them
    text = np.full(2 * 3, ord("A"), dtype=np.uint8)
    ok = _lib.GtreeTables(text=text, nrows=2, ncols=3)
    _lib.gtree_check(ok)
    emu.gtree_check(ok)
    for bad, code in ((_lib.GtreeTables(text=np.full((N + 1), 65, dtype=np.uint8), nrows=N + 1, ncols=1), -7),
                      (_lib.GtreeTables(text=np.full(2 * (L + 1), 65, dtype=np.uint8), nrows=2, ncols=L + 1), -7),
                      (_lib.GtreeTables(text=np.array([65, 200, 65, 65], dtype=np.uint8), nrows=2, ncols=2), -7),
                      (_lib.GtreeTables(text=text, nrows=2, ncols=3, cols=[[0, 1, 3]]), -1),
                      (_lib.GtreeTables(text=text, nrows=3, ncols=3), -1),
                      (_lib.GtreeTables(text=text, nrows=2, ncols=3, max_dist=0.0), -1),
                      (_lib.GtreeTables(text=text, nrows=2, ncols=3, max_dist=float("inf")), -1),
                      (_lib.GtreeTables(text=text, nrows=2, ncols=3, model=5), -1),
                      (_lib.GtreeTables(matrices=np.full((1, 2, 2), np.inf)), -1)):
        for check in (_lib.gtree_check, emu.gtree_check, _lib.gtree_host):
            with pytest.raises(_lib.CkmError) as e:
                check(bad)
            assert e.value.code == code


def test_abi_line_and_exports():
    header = open(os.path.join(ROOT, "include", "checkm_hip.h")).read()
    assert "#define CKM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12 and _lib.load().ckm_abi_version() == 12
    line = [ln for ln in header.split("\n") if ln.startswith("#define CKM_ABI_VERSION")][0]
    assert "ckm_gtree_*" in line and "ckm_select_*" in line
    for name in ("ckm_gtree_check", "ckm_gtree_host", "ckm_gtree_run"):
        assert name in _lib.EXPORTS and ("int  %s(" % name) in header and hasattr(_lib.load(), name)
