#!/usr/bin/env python
"""Goldens of ReducedTree's clusters: __nearlyIdenticalGenomes of scripts/genometreeworkflow/createSmallTree.py of the reference over
small alignments.  The script is Python 2 and does not compile as it stands; its class text is loaded in memory after the substitutions
listed below (each counted) and never written to disk.  The class is not constructed through its __init__ (which looks for FastTree and
for the authors' IMG tables): an instance is made bare and given an empty `metadata` stand-in, which the method only prints from.  The
rows go in as a dict in file order (the dicts of the running Python 3 keep it); a cluster is a set there, so the goldens hold every
cluster as a sorted list, in the order the clusters were made, and the membership of every line of nearly_identical.tsv likewise.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_reducedtree_golden.py [--time]      (writes tests/golden/reducedtree_cases.json;
       --time: the reference's loop on one core over a synthetic alignment, to profiles/r27_reducedtree_reference_cpu.json)"""
import contextlib
import io
import itertools
import json
import os
import random
import re
import sys
import tempfile
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_simulation_golden import translate                                                                        # noqa: E402

SUBSTITUTIONS = [("print statements", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)"), ("xrange", r"\bxrange\(", "range("), ("izip", r"itertools\.izip\(", "zip("),
                 ("indexable keys", r"\bseqs\.keys\(\)", "list(seqs.keys())")]
HITS = {"print statements": 17, "xrange": 2, "izip": 1, "indexable keys": 1}


def load_class(source):
    text = open(os.path.join(source, "scripts", "genometreeworkflow", "createSmallTree.py")).read()
    m = re.search(r"(?ms)^class CreateSamllTree\(object\):.*?(?=^if __name__)", text)
    if not m:
        raise SystemExit("class CreateSamllTree not found")
    ns = {"os": os, "sys": sys, "random": random, "itertools": itertools}
    exec(compile(translate(m.group(0), SUBSTITUTIONS, HITS), "<createSmallTree.py, translated in memory>", "exec"), ns)
    return ns["CreateSamllTree"]


def reference_clusters(cls, rows):
    """(clusters, tsv): rows [(id, text)] in file order through the reference's method in a fresh directory."""
    obj = object.__new__(cls)
    obj.metadata = defaultdict(lambda: {"taxonomy": ""})
    d = tempfile.mkdtemp(prefix="reducedtree_golden_")
    with contextlib.redirect_stdout(io.StringIO()):
        identical = obj._CreateSamllTree__nearlyIdenticalGenomes(dict(rows), d)
    with open(os.path.join(d, "nearly_identical.tsv")) as f:
        tsv = [sorted(x.strip() for x in line.split("\t")) for line in f]
    return [sorted(s) for s in identical], tsv


def mutate(rnd, row, ndiff, span=None):
    cols = rnd.sample(range(len(row)) if span is None else span, ndiff)
    out = list(row)
    for c in cols:
        out[c] = "C" if out[c] == "A" else "A"
    return "".join(out)


def cases():
    rnd = random.Random(29)
    letters = "ACDEFGHIKLMNPQRSTVWY-"
    draw = lambda n: "".join(rnd.choice(letters) for _ in range(n))
    out = []
    # limits 0 -> identical only, 1 -> identical only, 2 -> one difference allowed
    for n in (12, 13, 25):
        a = draw(n)
        out.append(("columns_%d" % n, [("a", a), ("b", mutate(rnd, a, 1)), ("c", a), ("d", mutate(rnd, a, 2)), ("e", draw(n)), ("f", mutate(rnd, a, 1, [n - 1]))]))
    # 100 columns, limit 8: 7 differences are near, 8 and 9 are not; first and last column among them
    a = draw(100)
    out.append(("columns_100", [("lead", a), ("seven", mutate(rnd, a, 7)), ("eight", mutate(rnd, a, 8)), ("nine", mutate(rnd, a, 9)), ("ends", mutate(rnd, a, 2, [0, 99])),
                                ("other", draw(100)), ("same", a)]))
    # not transitive: a ~ b (5), b ~ c (5), a !~ c (10); and the same rows in another order
    a = draw(100)
    b = mutate(rnd, a, 5, range(0, 50))
    c = mutate(rnd, b, 5, range(50, 100))
    out.append(("chain_abc", [("a", a), ("b", b), ("c", c)]))
    out.append(("chain_bac", [("b", b), ("a", a), ("c", c)]))
    # gaps, both cases of a letter and bytes beyond ASCII count as themselves
    a = draw(50)
    out.append(("raw_bytes", [("upper", a), ("lower", a.lower()), ("gaps", a[:47] + "---"), ("high", a[:47] + "\xe9\xff\x80"), ("high2", a[:47] + "\xe9\xff\x00"),
                              ("bit7", "".join(chr(ord(ch) | 0x80) for ch in a)), ("upper2", a)]))
    # unequal lengths: the reference's zip stops at the shorter row, the limit is the first row's
    a = draw(40)
    out.append(("unequal_lengths", [("long", a + draw(20)), ("short", a), ("short2", mutate(rnd, a, 2)), ("longer", a + draw(40)), ("empty", "")]))
    # all identical, all different, a single row
    out.append(("all_identical", [("g%d" % k, a) for k in range(6)]))
    out.append(("all_different", [("g%d" % k, draw(60)) for k in range(6)]))
    out.append(("one_row", [("only", a)]))
    # groups over more than one tile: 70 rows of 300 columns (limit 24)
    rows = []
    for g in range(10):
        lead = draw(300)
        rows.append(("g%d_0" % g, lead))
        for k, nd in enumerate((0, 23, 24, 25, 12, 40), 1):
            rows.append(("g%d_%d" % (g, k), mutate(rnd, lead, nd)))
    rnd.shuffle(rows)
    out.append(("seventy_rows", rows))
    return out


def time_reference(cls, rows=120, columns=6988):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import reducedtree_synth as synth
    text = synth.alignment(29, rows, columns)
    seqs = [(i, bytes(text[k]).decode("latin-1")) for k, i in enumerate(synth.ids_of(rows))]
    t0 = time.perf_counter()
    clusters, _ = reference_clusters(cls, seqs)
    dt = time.perf_counter() - t0
    out = {"what": "the reference's __nearlyIdenticalGenomes loop (text translated in memory), one core, tests/reducedtree_synth.alignment(29, rows, columns)",
           "rows": rows, "columns": columns, "clusters": len(clusters), "seconds": dt, "row_pairs_per_s": rows * (rows - 1) / 2 / dt}
    with open(os.path.join(ROOT, "profiles", "r27_reducedtree_reference_cpu.json"), "w") as f:
        f.write(json.dumps(out, sort_keys=True) + "\n")
    print(json.dumps(out, sort_keys=True))


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    if not os.path.isdir(os.path.join(source, "scripts", "genometreeworkflow")):
        raise SystemExit("set CHECKM_SOURCE to the CheckM source tree")
    cls = load_class(source)
    if "--time" in sys.argv[1:]:
        return time_reference(cls)
    out = []
    for name, rows in cases():
        clusters, tsv = reference_clusters(cls, rows)
        out.append({"name": name, "rows": [list(r) for r in rows], "clusters": clusters, "tsv": tsv})
    path = os.path.join(ROOT, "tests", "golden", "reducedtree_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
