#!/usr/bin/env python
"""Goldens of the placement (tests/golden/placement_cases.json).

"recovery": a random tree of 16 leaves with lengths U[0.08, 0.3] under a trifurcating root, 400 sites simulated down it under a seeded
random reversible 20-state model with rates (0.3, 1.7), pendant grid (0.01, 0.03, 0.1, 0.3, 1.0) and distal fractions (1/8, 3/8, 5/8,
7/8).  Every leaf is pruned and must go back on the merged edge it came from.  Before anything is written the brute-force formulation
of tests/emu/placement_oracle.py (the query inserted in the tree, scipy.linalg.expm for every P(t)) must recover all leaves with a
margin of at least 1.0 log units between the best and the second edge; a seed that does not is passed over for the next.

"concat": what the reference's own PplacerRunner._createConcatenatedAlignment (checkm/pplacer.py:89-132) writes for small directories of
*.masked.faa files, as the parsed {binId: sequence} and the record format.  The reference's class is instantiated without its
constructor (which looks for the pplacer and guppy programs); its method runs unchanged.  This is the only place the reference is read.
Runs only where a CheckM source tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_placement_golden.py"""
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from checkm_amd.pplacer import nodes_of, parse_newick, plain_name      # noqa: E402
from tests.emu import placement_oracle as orc                          # noqa: E402

PENDANT = (0.01, 0.03, 0.1, 0.3, 1.0)
DISTAL = (0.125, 0.375, 0.625, 0.875)
RATES, WEIGHTS = (0.3, 1.7), (0.5, 0.5)
NLEAVES, NSITES, MARGIN = 16, 400, 1.0


def recovery_case(seed):
    rng = np.random.default_rng(seed)
    S, pi = orc.random_model(rng)
    text = orc.random_tree(rng, NLEAVES, 0.08, 0.3, root_degree=3)
    aln = orc.simulate(rng, parse_newick(text), S, pi, RATES, WEIGHTS, NSITES)
    oracle = orc.Oracle(S, pi, RATES, WEIGHTS)
    leaves, smallest = [], None
    for leaf in sorted(aln):
        pruned, want = orc.prune_leaf(text, leaf)
        root = parse_newick(pruned)
        rest = {k: v for k, v in aln.items() if k != leaf}
        per_edge = {}
        for v in nodes_of(root):
            if v.parent is None:
                continue
            per_edge[v.num] = max(oracle.placed(root, rest, aln[leaf], v.num, f * float(v.length), b) for f in DISTAL for b in PENDANT)
        ranked = sorted(per_edge, key=lambda e: -per_edge[e])
        others = [e for e in ranked if e not in want]
        margin = per_edge[ranked[0]] - per_edge[others[0]]
        if ranked[0] not in want or margin < MARGIN:
            return None
        smallest = margin if smallest is None else min(smallest, margin)
        leaves.append(dict(leaf=leaf, tree=pruned, edges=want, oracle_logL=per_edge[ranked[0]], oracle_margin=margin))
    iu = [(i, j) for i in range(1, 20) for j in range(i)]
    return dict(seed=seed, tree=text, alignment=aln, exchangeabilities=[float(S[i, j]) for i, j in iu], frequencies=[float(x) for x in pi], rates=list(RATES),
                weights=list(WEIGHTS), pendant=list(PENDANT), distal=list(DISTAL), leaves=leaves, smallest_margin=smallest)


CONCAT_CASES = {
    "two_markers_one_missing": dict(lengths={"PF00001.1": 7, "TIGR00002": 5},
                                    files={"PF00001.1": {"binA&&c1_3": "MKV-LLA", "binB&&c9_1": "MRV-LIA"}, "TIGR00002": {"binA&&c2_8": "GG-SA"}}),
    "bin_seen_in_one_marker": dict(lengths={"A": 3, "B": 4, "C": 2},
                                   files={"A": {"x&&1": "AAA"}, "B": {"x&&2": "CCCC", "y&&7": "DD-D"}, "C": {"x&&3": "EE"}}),
    "marker_without_file": dict(lengths={"M1": 4, "M2": 3}, files={"M1": {"b1&&g": "WWWW", "b2&&g": "YYYY"}}),
    "nothing": dict(lengths={"M1": 4}, files={}),
}


def concat_cases(source):
    sys.path.insert(0, source)
    home = tempfile.mkdtemp()
    os.environ["HOME"] = home                                      # the reference's package writes a settings folder at import
    import checkm.pplacer as ref
    out = {}
    for name, case in sorted(CONCAT_CASES.items()):
        d = tempfile.mkdtemp()
        for marker, seqs in case["files"].items():
            with open(os.path.join(d, marker + ".masked.faa"), "w") as f:
                for seq_id, seq in seqs.items():
                    f.write(">%s\n%s\n" % (seq_id, seq))
        runner = ref.PplacerRunner.__new__(ref.PplacerRunner)
        runner.logger = logging.getLogger("golden")
        parser = types.SimpleNamespace(models={"bin": {m: types.SimpleNamespace(leng=n) for m, n in case["lengths"].items()}})
        path = runner._createConcatenatedAlignment([], parser, d)
        text = open(path).read()
        lines = text.split("\n")
        assert text == "" or (text.endswith("\n") and all(ln.startswith(">") for ln in lines[0:-1:2]))
        out[name] = dict(case, file=os.path.basename(path), seqs={lines[k][1:]: lines[k + 1] for k in range(0, len(lines) - 1, 2)})
    return out


def main():
    source = os.environ.get("CHECKM_SOURCE")
    if not source:
        raise SystemExit("CHECKM_SOURCE is not set")
    seed, case = 2, None
    while case is None:
        case = recovery_case(seed)
        print("seed %d: %s" % (seed, "recovered, smallest margin %.2f" % case["smallest_margin"] if case else "passed over"))
        seed += 1
    path = os.path.join(ROOT, "tests", "golden", "placement_cases.json")
    with open(path, "w") as f:
        json.dump({"generator": "tools/gen_placement_golden.py", "reference": "checkm/pplacer.py (v1.2.4) _createConcatenatedAlignment", "recovery": case,
                   "concat": concat_cases(source)}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
