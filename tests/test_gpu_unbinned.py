"""Unbinned on the device: kernels_unbinned.hip against the reference's goldens (tests/golden/unbinned_cases.json) through the full `run`,
and ckm_unbinned_count against the host executor (tests/emu/unbinned_emu.cpp) and the byte-wise restatement.  Everything is compared
at ==; nothing is timed."""
import ctypes as C

import numpy as np
import pytest

from checkm_amd import _lib
from tests.emu import unbinned as emu
from tests.test_unbinned_host import CASES, base_count, check_case

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 5]


def synthetic():
    """A few hundred sequences (str): every length of LENS in every flavour, and multi-byte characters placed across the 16-byte chunk
    seam (bytes 15 | 16) and the tile seams of 1 KiB and 4 KiB (bytes 1023 | 1024 and 4095 | 4096 of the sequence)."""
    rng = np.random.default_rng(19)
    flavours = ["ACGT", "acgt", "ACGTacgtUuNn", "NnACGTXxRYKM-*"]
    seqs = []
    for rep in range(5):
        for L in LENS:
            for f in flavours:
                seqs.append("".join(rng.choice(list(f), L)) if L else "")
    for L in (17, 1025, 4097, 3 * 4096 + 5):
        for ch in ("é", "€", "\U0001F9EC"):               # 2, 3 and 4 bytes
            for seam in (16, 1024, 4096):
                if seam + 8 > L:
                    continue
                body = "".join(rng.choice(list("ACGTacgtu"), L))
                n = len(ch.encode("utf-8"))
                for first in range(1, n):                           # `first` bytes of the character lie in front of the seam
                    s = body[:seam - first] + ch + body[seam - first:]
                    assert s.encode("utf-8")[seam - first:seam - first + n] == ch.encode("utf-8")
                    seqs.append(s)
    return seqs


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the batch, per-sequence restatement [nseq, 5]) of the synthetic assembly, read once."""
    seqs = synthetic()
    path = str(tmp_path_factory.mktemp("unbinned_gpu") / "assembly.fna")
    open(path, "w", encoding="utf-8").write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    b = _lib.NucSeqs([path])
    assert b.nseq == len(seqs) and 200 <= b.nseq <= 999
    want = np.array([base_count(s.encode("utf-8")) for s in seqs], dtype=np.uint64)
    assert want[:, 4].tolist() == [len(s) for s in seqs] and (want[:, 4] != b.seq_bytes).sum() > 20
    yield b, want
    b.close()


@pytest.mark.parametrize("name", list(CASES))
def test_run_reproduces_the_reference(gpu_ctx, tmp_path, name):
    u = check_case(tmp_path, CASES[name])
    if CASES[name]["error"] is None:
        assert u.last_timing["batches"] == (1 if u.last_timing["tiles"] else 0)


def test_device_count_against_the_host_executor_and_the_restatement(gpu_ctx, assembly):
    b, want = assembly
    n = b.nseq
    padded = (b.seq_bytes + 15) // 16 * 16
    first = None
    for keep in (np.ones(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), (np.arange(n) % 2 == 0).astype(np.uint8)):
        expect = (want * keep[:, None]).tolist()
        total = int((padded * keep).sum())                        # a quarter of the kept text per batch: at least four batches
        for tile in (1024, 4096):
            for budget in (total // 4, 1 << 30):
                r = _lib.unbinned_count(gpu_ctx, b, keep, tile_bytes=tile, budget_bytes=budget)
                e = emu.unbinned_count(None, b, keep, tile_bytes=tile, budget_bytes=budget)
                assert r["counts"].tolist() == expect and e["counts"].tolist() == expect
                assert (r["kept"], r["tiles"], r["batches"], r["bytes"]) == (e["kept"], e["tiles"], e["batches"], e["bytes"])
                assert r["batches"] >= 3 if budget < 1 << 30 else r["batches"] == 1
                if first is None:
                    first = r["counts"].copy()
    again = _lib.unbinned_count(gpu_ctx, b, np.ones(n, np.uint8), tile_bytes=1024, budget_bytes=int(padded.sum()) // 4)
    assert again["counts"].tobytes() == first.tobytes()
    assert _lib.unbinned_count(gpu_ctx, b, np.ones(n, np.uint8))["counts"].tobytes() == first.tobytes()      # the default tile and budget


def test_nothing_kept_launches_nothing(gpu_ctx, assembly):
    b, _want = assembly
    r = _lib.unbinned_count(gpu_ctx, b, np.zeros(b.nseq, np.uint8))
    assert not r["counts"].any() and (r["kept"], r["tiles"], r["batches"], r["bytes"]) == (0, 0, 0, 0)
    only_empty = (b.seq_bytes == 0).astype(np.uint8)
    r = _lib.unbinned_count(gpu_ctx, b, only_empty)
    assert not r["counts"].any() and r["kept"] == int(only_empty.sum()) > 0 and r["batches"] == 0


def test_bad_arguments_are_refused(gpu_ctx, assembly):
    b, _want = assembly
    keep = np.ones(b.nseq, np.uint8)
    for tile in (1000, 16, 1536, (1 << 20) + 1024):
        with pytest.raises(_lib.CkmError) as e:
            _lib.unbinned_count(gpu_ctx, b, keep, tile_bytes=tile)
        assert e.value.code == -1
    counts = np.zeros((b.nseq, 5), dtype=np.uint64)
    t = _lib.UnbinnedTiming()
    L = _lib.load()
    for args in ((None, b.h, keep.ctypes.data, 0, 0, counts.ctypes.data, C.byref(t)), (gpu_ctx.h, None, keep.ctypes.data, 0, 0, counts.ctypes.data, C.byref(t)),
                 (gpu_ctx.h, b.h, None, 0, 0, counts.ctypes.data, C.byref(t)), (gpu_ctx.h, b.h, keep.ctypes.data, 0, 0, None, C.byref(t)),
                 (gpu_ctx.h, b.h, keep.ctypes.data, 0, 0, counts.ctypes.data, None)):
        assert L.ckm_unbinned_count(*args) == -1
    assert not counts.any()
