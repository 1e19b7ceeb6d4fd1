"""The all-pairs amino-acid identity on the device: kernels_aai.hip against the host executor (tests/emu/aai_emu.cpp) and the plain
restatement of aai() on the synthetic set of tests/test_aai_host.py, and the reference's goldens (tests/golden/aai_cases.json) through
the real `run`.  mismatches, compared and the bits of aai are compared at ==; nothing is timed."""
import pytest

from checkm_amd import _lib
from tests.emu import aai as emu
from tests.test_aai_host import CASES, TAKES, TIMING_KEYS, check_case, equals, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """(groups, restatement, the host executor's result in one batch): computed once for the module."""
    groups, want = synthetic()
    return groups, want, emu.aai_pairs(None, groups, budget_bytes=1 << 30)


def same(r, e):
    return all(r[f].tobytes() == e[f].tobytes() for f in ("pair_off", "mismatches", "compared", "aai")) and r["npairs"] == e["npairs"]


def test_device_against_the_host_executor_and_the_restatement(gpu_ctx, expected):
    groups, want, e = expected
    r = _lib.aai_pairs(gpu_ctx, groups, budget_bytes=1 << 30)
    assert equals(r, want) and equals(e, want) and same(r, e)
    assert (r["nbatches"], r["bytes"]) == (e["nbatches"], e["bytes"]) == (1, e["bytes"])


def test_batches_do_not_change_a_result(gpu_ctx, expected):
    groups, want, e = expected
    budget = (e["bytes"] + 16 * len(want)) // 3                      # a third of the text and the outputs: at least three batches
    cut = _lib.aai_pairs(gpu_ctx, groups, budget_bytes=budget)
    c = emu.aai_pairs(None, groups, budget_bytes=budget)
    assert cut["nbatches"] == c["nbatches"] >= 3 and cut["bytes"] == c["bytes"]
    assert same(cut, e) and equals(cut, want)
    again = _lib.aai_pairs(gpu_ctx, groups, budget_bytes=budget)
    assert same(again, cut)                                          # a repeated call: the same bits
    assert same(_lib.aai_pairs(gpu_ctx, groups), e)                  # the default budget


def test_calls_without_a_pair_and_refused_calls(gpu_ctx):
    r = _lib.aai_pairs(gpu_ctx, [[], [b"ACD"], []])
    assert r["npairs"] == 0 and r["nbatches"] == 0 and r["pair_off"].tolist() == [0, 0, 0, 0] and len(r["aai"]) == 0
    assert _lib.aai_pairs(gpu_ctx, [])["npairs"] == 0
    for groups, code in (([[b"ACD", b"AC"]], -1), ([[b"A" * 4097, b"C" * 4097]], -7)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.aai_pairs(gpu_ctx, groups)
        assert e.value.code == code


@pytest.mark.parametrize("name", list(CASES))
def test_run_reproduces_the_reference(gpu_ctx, tmp_path, monkeypatch, name):
    a = check_case(tmp_path, CASES[name], monkeypatch)
    assert set(a.last_timing) >= TIMING_KEYS
    assert (a.last_timing["groups"], a.last_timing["pairs"]) == TAKES[name]          # the device took them: no group fell to the host loop
    assert a.last_timing["batches"] == (1 if TAKES[name][0] else 0)
