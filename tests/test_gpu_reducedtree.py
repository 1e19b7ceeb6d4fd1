"""The near-identity pass on the device: the kernel of libcheckm_hip (kernels_nearid.hip) against the host executor of the same header
(ckm_nearid_host) at == on the whole bit matrix, on the smallest shapes that can still break: row counts 1, 2, 63, 64, 65, 129 and 200 (a
single tile, a ragged last tile, diagonal and off-diagonal tiles), row lengths 1, 7, 8, 9, 12, 13, 25, 127, 128, 129 and 300 (word and
chunk edges, limits 1, 1, 2, ...), planted pairs at exactly limit - 1, limit and limit + 1 differences (in the first byte, the last byte
of a row, the last byte of a 64-bit word, or spread over several chunks so that an early exit is crossed), every byte value but newline,
pairs that differ in bit 7 alone, identical rows, all-different rows, per-row limits that differ within a tile; three budgets, one of
which gives a band per row tile; the goldens through ReducedTree's default device path with no fallback; and one run from derep FASTA
and tree to the four files."""
import json
import os
import random

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.genomeTree import readFasta
from checkm_amd.reducedTree import ReducedTree
from checkm_amd.treeParser import read_newick
from tests.emu import nearid as emu
from tests.test_reducedtree_host import ROW_COUNTS, ROW_LENGTHS, planted, shapes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "reducedtree_cases.json")))


def budgets(t):
    """one band per row tile; two row tiles per band; the default"""
    return (1, t.n_rows * t.row_stride + t.n_rows * 4 + 2 * 64 * t.words * 8, 0)


def test_shapes_are_the_ones_named():
    assert sorted(set(n for n, _ in shapes())) == sorted(ROW_COUNTS) and sorted(set(L for n, L in shapes() if n == 65)) == sorted(ROW_LENGTHS)


@pytest.mark.parametrize("n_rows,row_len", shapes())
def test_device_equals_the_host_executor(gpu_ctx, n_rows, row_len):
    text, limit = planted(n_rows * 1000 + row_len, n_rows, row_len)
    t = _lib.NearidTables(text, limit)
    want = _lib.nearid_host(t)
    for budget in budgets(t):
        got = _lib.nearid_run(gpu_ctx, t, budget)
        assert got["near"].tolist() == want["near"].tolist(), budget
        assert got["nbands"] == len(emu.bands(n_rows, t.row_stride, budget if budget else 256 << 20)) and got["launches"] == got["nbands"]
        tiles = (n_rows + 63) // 64
        assert got["blocks"] == tiles * (tiles + 1) // 2 and got["npairs"] == n_rows * (n_rows - 1) // 2
    assert [b for b in (len(emu.bands(n_rows, t.row_stride, x)) for x in budgets(t)[:2])] == [(n_rows + 63) // 64, ((n_rows + 63) // 64 + 1) // 2]


def test_identical_rows_and_all_different_rows(gpu_ctx):
    same = np.tile(np.arange(1, 201, dtype=np.uint8) | 1, (130, 1))
    t = _lib.NearidTables(same, np.ones(130))
    got = _lib.nearid_run(gpu_ctx, t)["near"]
    assert got.tolist() == _lib.nearid_host(t)["near"].tolist() == emu.near_bits(same, np.ones(130)).tolist()
    assert got[0].tolist() == [0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF, 0x3] and got[129].tolist() == [0, 0, 0] and got[64].tolist() == [0, 0xFFFFFFFFFFFFFFFE, 0x3]
    different = ((np.arange(130)[:, None] + np.arange(200)[None, :] * 0) % 251 + 1).astype(np.uint8)      # row i holds i + 1 in every column
    for limit in (np.full(130, 200), np.full(130, 201)):
        t = _lib.NearidTables(different, limit)
        got = _lib.nearid_run(gpu_ctx, t, 1)["near"]
        assert got.tolist() == _lib.nearid_host(t)["near"].tolist()
        assert bool(got.any()) == (int(limit[0]) == 201)


def test_every_byte_value_and_bit_seven(gpu_ctx):
    base = np.arange(256, dtype=np.uint8)
    text = np.stack([base, base ^ 0x80, base ^ 0x01, base, np.zeros(256, dtype=np.uint8)] + [np.roll(base, k) for k in range(1, 70)])
    for limit in ([257, 256, 1, 1, 1] + [3] * 69, [256, 257, 1, 1, 1] + [256] * 69):
        t = _lib.NearidTables(text, limit)
        got = _lib.nearid_run(gpu_ctx, t)["near"]
        assert got.tolist() == _lib.nearid_host(t)["near"].tolist() == emu.near_bits(text, limit).tolist()
        assert int(got[0, 0]) & 0b11110 in (0b11110, 0b11000)


def test_refused_before_any_launch(gpu_ctx):
    text = np.zeros((3, 20), dtype=np.uint8)
    with pytest.raises(_lib.CkmError) as e:
        _lib.nearid_run(gpu_ctx, _lib.NearidTables(text, [1, 0, 1]))
    assert e.value.code == -1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_goldens_through_the_default_device_path(gpu_ctx, case):
    rows = {k: s for k, s in case["rows"]}
    equal = len(set(len(s) for s in rows.values())) == 1 and all(rows.values())
    r = ReducedTree()
    got = r.nearlyIdentical(rows)
    assert [sorted(x) for x in got] == case["clusters"]
    assert r.lastInfo["python_fallbacks"] == (0 if equal else 1)
    if equal:
        assert r.lastInfo["launches"] >= 1


def test_run_on_a_small_directory(gpu_ctx, tmp_path, capsys):
    rnd = random.Random(11)
    letters = "ACDEFGHIKLMNPQRSTVWY-"
    rows = []
    for g in range(6):
        lead = "".join(rnd.choice(letters) for _ in range(200))
        rows.append(("IMG_%d0" % g, lead))
        for k, nd in enumerate((0, 15, 16, 40)[:1 + g % 4], 1):                        # limit 16: 0 and 15 differences join the lead's cluster
            row = list(lead)
            for c in rnd.sample(range(200), nd):
                row[c] = "A" if row[c] != "A" else "C"
            rows.append(("IMG_%d%d" % (g, k), "".join(row)))
    src, out = tmp_path / "full", tmp_path / "reduced"
    os.makedirs(src)
    open(src / "genome_tree.concatenated.derep.fasta", "w").write("".join(">%s\n%s\n" % r for r in rows))
    nodes = ["%s:%r" % (k, round(rnd.random(), 3)) for k, _ in rows]
    n = 0
    while len(nodes) > 1:
        a, b = nodes.pop(rnd.randrange(len(nodes))), nodes.pop(rnd.randrange(len(nodes)))
        n += 1
        nodes.append("(%s,%s)'UID%d|k__X;p__Y|0.9':%r" % (a, b, n, round(rnd.random(), 3)))
    open(src / "genome_tree.final.tre", "w").write(nodes[0].rsplit(":", 1)[0] + ";\n")
    random.seed(3)
    r = ReducedTree()
    kept = r.run(str(src), str(out))
    assert r.lastInfo["python_fallbacks"] == 0 and "Missing taxa" not in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["genome_tree.fasta", "genome_tree.small.no_internal_labels.tre", "genome_tree.tre", "nearly_identical.tsv"]
    clusters = [line.rstrip("\n").split("\t") for line in open(out / "nearly_identical.tsv")]
    want = ReducedTree(runner=_lib.nearid_host).nearlyIdentical(dict(rows))
    assert clusters == want and sorted(len(c) for c in clusters) == [1, 1, 1, 2, 2, 3, 3, 3, 3]
    fasta = readFasta(str(out / "genome_tree.fasta"))
    assert list(fasta) == kept and len(kept) == len(clusters) and all(k in c and fasta[k] == dict(rows)[k] for k, c in zip(kept, clusters))
    tree, bare = read_newick(open(out / "genome_tree.tre").read()), read_newick(open(out / "genome_tree.small.no_internal_labels.tre").read())
    assert sorted(leaf.taxon for leaf in tree.root.leaves()) == sorted(kept) == sorted(leaf.taxon for leaf in bare.root.leaves())
    labels, bare_labels = [], []
    for root, into in ((tree.root, labels), (bare.root, bare_labels)):
        stack = [root]
        while stack:
            v = stack.pop()
            stack.extend(v.children)
            if v.children:
                assert len(v.children) >= 2
                into.append(v.label)
    assert all(x.startswith("UID") for x in labels) and set(bare_labels) == {""}
    random.seed(3)
    again = ReducedTree().run(str(src), str(out))                                       # resumes from nearly_identical.tsv; the same seed, the same choice
    assert again == kept
