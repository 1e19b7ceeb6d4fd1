"""The stream plan (csrc/stream_plan.h): which stream of the per-device pool every logical stream of a search context uses, by the number of
hardware queues the process runs with.  The header is pure host code; it is compiled here into a ctypes shim of its own."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "checkm_amd", "csrc", "stream_plan.h")
NCTX, NSIDE = 3, 14          # context slots and side streams of a plan (kPlanContexts, kPlanSide)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler to build the plan shim with"
    d = tmp_path_factory.mktemp("stream_plan")
    src = d / "shim.cpp"
    src.write_text('#define CKM_STREAM_PLAN_SHIM 1\n#include "%s"\n' % HEADER)
    so = d / "libstream_plan.so"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-x", "c++", str(src), "-o", str(so)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lib = C.CDLL(str(so))
    lib.ckm_plan_queue_budget.argtypes = [C.c_char_p, C.c_char_p]
    lib.ckm_plan_queue_budget.restype = C.c_int
    lib.ckm_plan_fill.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.ckm_plan_fill.restype = None
    return lib


def plan(lib, budget, contexts):
    buf = (C.c_int * (3 + NCTX * 16))()
    lib.ckm_plan_fill(budget, contexts, buf)
    v = list(buf)
    p = {"nhandles": v[0], "nss": v[1], "nch": v[2], "ctx": []}
    for c in range(NCTX):
        row = v[3 + 16 * c: 3 + 16 * (c + 1)]
        p["ctx"].append({"main": row[0], "side": row[1:15], "ens": row[15]})
    return p


def roles(p, contexts):
    """handles by role over the contexts in flight: SSV, chain, ensembles, main"""
    ssv, chain, ens, main = set(), set(), set(), set()
    for c in range(contexts):
        x = p["ctx"][c]
        ssv.update(x["side"][:p["nss"]])
        chain.update(x["side"][p["nss"]:p["nss"] + p["nch"]])
        ens.add(x["ens"])
        main.add(x["main"])
    return ssv, chain, ens, main


@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("budget", list(range(1, 33)))
def test_every_stream_mapped_within_budget(shim, budget, contexts):
    p = plan(shim, budget, contexts)
    assert 1 <= p["nss"] <= 4 and 0 <= p["nch"] <= 10
    assert 1 <= p["nhandles"] <= budget
    used = set()
    for c in range(NCTX):                      # every slot is mapped, also those beyond the contexts in flight (they wrap)
        x = p["ctx"][c]
        for h in [x["main"], x["ens"]] + x["side"]:
            assert 0 <= h < p["nhandles"]
        used.update([x["main"], x["ens"]] + x["side"])
        n = p["nss"] + p["nch"]
        assert len(set(x["side"][:n])) == n                        # the distinct side streams come first ...
        assert set(x["side"][n:]) <= set(x["side"][:n])            # ... and the rest alias them
    assert len(used) <= budget
    assert used == set(range(p["nhandles"]))                       # the pool creates no stream that nothing uses
    ssv, chain, ens, main = roles(p, contexts)
    if budget >= 2:
        # an SSV handle carries SSV launches only
        assert p["nch"] >= 1
        assert not ssv & chain and not ssv & ens
    if 2 <= budget < 16:
        assert not ssv & main
    if 2 <= budget <= 4:
        # few queues: one SSV handle, every other one a chain handle; main stream and ensembles on the last of them
        assert (p["nss"], p["nch"]) == (1, budget - 1)
        assert main == ens == {budget - 1}
    if 5 <= budget < 16:
        assert p["nch"] >= 3 and len(main) == 1 and not main & chain
    if 6 <= budget < 16:
        # the ensembles do not sit in front of a chain once a separate handle exists
        assert not ens & chain and not ens & main
    if budget < 16:
        assert p["nhandles"] == budget                             # no queue is left without a stream


@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("budget", list(range(1, 16)))
def test_chains_share_handles_in_launch_order(shim, budget, contexts):
    """below 16 queues the groups of every context go round the same chain handles (their SSV launches finish in launch order)"""
    p = plan(shim, budget, contexts)
    n = p["nss"] + p["nch"]
    for c in range(1, NCTX):
        assert p["ctx"][c]["side"][:n] == p["ctx"][0]["side"][:n]
    assert p["ctx"][0]["side"][:n] == list(range(n))               # creation order: SSV handles, then chain handles


@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("budget", list(range(16, 33)))
def test_sixteen_queues_or_more_is_the_mapping_there_always_was(shim, budget, contexts):
    """1 main + 14 side (4 SSV, 10 chain) + 1 ensemble stream per context, in the order ckm_ctx_create made them: main, side[0 .. 14), ensembles.
    Launch g of a search goes to side[g % 4], its chain to side[4 + g % 10]."""
    p = plan(shim, budget, contexts)
    assert (p["nss"], p["nch"]) == (4, 10)
    nslots = min(budget // 16, contexts)
    assert p["nhandles"] == 16 * nslots
    for c in range(contexts):
        base = 16 * (c % nslots)
        assert p["ctx"][c] == {"main": base, "side": [base + 1 + k for k in range(14)], "ens": base + 15}
    if budget >= 32 and contexts >= 2:
        a, b = p["ctx"][0], p["ctx"][1]
        assert not set([a["main"], a["ens"]] + a["side"]) & set([b["main"], b["ens"]] + b["side"])


def test_plan_by_budget_below_sixteen(shim):
    """(SSV, chain, own ensemble handle, own main handle) by budget, as DESIGN.md section 5 tabulates it; HIP's default of 4 queues: 1 + 3"""
    want = {1: (1, 0, 0, 0), 2: (1, 1, 0, 0), 3: (1, 2, 0, 0), 4: (1, 3, 0, 0), 5: (1, 3, 0, 1), 6: (1, 3, 1, 1), 7: (1, 4, 1, 1), 8: (2, 4, 1, 1),
            9: (2, 5, 1, 1), 10: (2, 6, 1, 1), 11: (2, 7, 1, 1), 12: (3, 7, 1, 1), 13: (3, 8, 1, 1), 14: (3, 9, 1, 1), 15: (4, 9, 1, 1)}
    for budget, (nss, nch, ens_own, main_own) in want.items():
        for contexts in (1, 2, 3):
            p = plan(shim, budget, contexts)
            ns = nss + nch
            assert (p["nss"], p["nch"], p["nhandles"]) == (nss, nch, ns + ens_own + main_own), budget
            for c in range(NCTX):
                assert p["ctx"][c]["ens"] == (ns if ens_own else ns - 1), budget
                assert p["ctx"][c]["main"] == (ns + ens_own if main_own else ns - 1), budget


def test_queue_budget(shim):
    f = shim.ckm_plan_queue_budget
    assert f(None, None) == 16                                     # nothing inherited: the 16 the library sets
    assert f(None, b"4") == 4
    assert f(b"6", b"4") == 6                                      # CKM_HW_QUEUES: what the host says HIP was started with
    assert f(b"", b"8") == 8
    assert f(None, b"0") == 1 and f(None, b"-3") == 1
    assert f(None, b"64") == 32 and f(b"1000", None) == 32
    assert f(None, b"abc") == 16
