"""The index arithmetic of a launch over a queue set (csrc/queue_set.h): the exclusive prefix of the queues' lengths, each clamped to its
capacity, and the map from a flat item number to (queue, position in it) that every wavefront of the float stages uses to find its work.
The header is compiled for the host and for the device; here tests/native/queue_set_check.cpp is compiled with AddressSanitizer and UBSan,
run as a child process on a case file, and held against a restatement in Python.  No device needed."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "checkm_amd", "csrc")
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("queue_set")
    exe = str(d / "queue_set_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "queue_set_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe, d


def run(harness, queues, ks):
    """queues: (count, cap) per queue"""
    exe, d = harness
    path = str(d / "case.txt")
    with open(path, "w") as f:
        f.write("%d\n%s\n%d\n%s\n" % (len(queues), " ".join("%d %d" % q for q in queues), len(ks), " ".join(map(str, ks))))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, **ENV))
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return json.loads(out.stdout)


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------------
def flat(queues):
    """the items of the set in flat order: every queue's existing entries (a producer that found the queue full still counted), queue by queue"""
    return [(q, pos) for q, (count, cap) in enumerate(queues) for pos in range(min(count, cap))]


def boundaries(queues):
    """0, every prefix boundary and its neighbours, the total and the numbers behind it"""
    pre = [0]
    for count, cap in queues:
        pre.append(pre[-1] + min(count, cap))
    ks = {0, pre[-1], pre[-1] + 1, 0xffffffff}
    for b in pre:
        ks |= {max(b - 1, 0), b, b + 1}
    return pre, sorted(ks)


def check(harness, queues, ks=None):
    pre, edge = boundaries(queues)
    ks = edge if ks is None else ks
    got = run(harness, queues, ks)
    items = flat(queues)
    assert got["pre"] == pre and got["total"] == pre[-1] == len(items)
    assert len(got["at"]) == len(ks)
    for k, (found, q, pos) in zip(ks, got["at"]):
        if k < len(items):
            assert (found, q, pos) == (1,) + items[k], k
            assert pos < min(queues[q])                    # never an entry beyond the count or the capacity, never an empty queue
        else:
            assert (found, q, pos) == (0, -1, -1), k       # no item: the outputs are left alone
    return got


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def test_one_queue_is_todays_single_queue(harness):
    got = check(harness, [(5, 9)])
    assert got["pre"] == [0, 5]
    assert got["at"][:2] == [[1, 0, 0], [1, 0, 1]]
    check(harness, [(5, 9)], ks=list(range(8)))
    check(harness, [(9, 5)], ks=list(range(8)))            # the count beyond the capacity: five entries exist


def test_three_queues_empty_one_and_clamped(harness):
    cap = 7
    queues = [(0, 4), (1, 4), (cap + 5, cap)]              # the third count exceeds its capacity: the clamp must hold
    got = check(harness, queues)
    assert got["pre"] == [0, 0, 1, 1 + cap] and got["total"] == 1 + cap
    every = run(harness, queues, list(range(cap + 4)))["at"]
    assert every[0] == [1, 1, 0]                           # flat 0 is the second queue's entry: the empty first queue is passed over
    assert every[1:1 + cap] == [[1, 2, p] for p in range(cap)]
    assert every[1 + cap:] == [[0, -1, -1]] * 3            # the entries the third queue counted and does not hold are no items


def test_all_queues_empty(harness):
    for n in (1, 3, 64, 192):
        got = check(harness, [(0, 8)] * n)
        assert got["total"] == 0 and not any(a[0] for a in got["at"])
    check(harness, [(3, 0), (0, 0)])                       # capacity 0: nothing exists whatever was counted
    assert run(harness, [], [0, 1])["at"] == [[0, -1, -1]] * 2


def test_192_queues_of_one_item(harness):
    queues = [(1, 1)] * 192
    check(harness, queues)
    got = run(harness, queues, list(range(194)))
    assert got["at"][:192] == [[1, q, 0] for q in range(192)] and got["at"][192:] == [[0, -1, -1]] * 2


def test_every_flat_number_of_a_mixed_set(harness):
    """lengths 0 .. 70 and back, runs of empty queues at both ends and in the middle, some counts beyond their capacities"""
    queues = [(0, 3)] * 2 + [(k, 64) for k in range(0, 71, 7)] + [(0, 1)] * 5 + [(90 - k, 33) for k in range(0, 90, 9)] + [(4, 4), (0, 9)]
    items = flat(queues)
    check(harness, queues)
    check(harness, queues, ks=list(range(len(items) + 3)))
