"""TEST INFRASTRUCTURE: synthetic gene trees and IMG metadata for the GeneTrees tests (tests/test_genetrees_host.py,
tests/test_gpu_genetrees.py).  Newick texts are built without recursion, so a caterpillar of thousands of leaves is fine."""
import os
import random

SPECIES = ("alpha", "beta", "Gamma", "", "unclassified")


def metadata(ngenomes, nphyla=3, nclasses=5, one_class=False, distinct=False, uncounted=False, prefix="G"):
    """{genome: {'taxonomy': seven ranks}} for <prefix>0 .. <prefix><n-1>.  one_class: one domain, phylum and class for every genome; distinct: a class
    of its own per genome at every rank; uncounted: no genome has a counted species."""
    md = {}
    for k in range(ngenomes):
        if one_class:
            tax = ["Bacteria", "P0", "C0"]
        elif distinct:
            tax = ["D%d" % k, "P%d" % k, "C%d" % k]
        else:
            tax = ["Archaea" if k % 7 == 3 else "Bacteria", "unclassified" if k % 11 == 5 else "P%d" % (k % nphyla), "C%d" % (k % nclasses)]
        genus = "unclassified" if k % 13 == 6 else "Genus%d" % (k % 4)
        species = "unclassified" if uncounted else SPECIES[k % len(SPECIES)]
        md["%s%d" % (prefix, k)] = {"taxonomy": tax + ["O", "F", genus, species]}
    return md


def labels(nleaves, ngenomes, rnd, copies=(), prefix="G"):
    """nleaves labels 'G<k>|c<n>'.  copies: (genome, count) pairs placed first; the rest cycle through the genomes; then shuffled."""
    out = []
    for g, count in copies:
        out += ["%s%d|p%d" % (prefix, g, k) for k in range(count)]
    k = 0
    while len(out) < nleaves:
        out.append("%s%d|c%d" % (prefix, k % ngenomes, k))
        k += 1
    rnd.shuffle(out)
    return out


def _length(rnd, zero):
    return "0.0" if rnd.random() < zero else repr(round(rnd.random(), 3))


def newick(shape, labs, rnd, zero=0.1):
    """shape: 'caterpillar', 'balanced', 'star', 'random' (multifurcations and single-child nodes) or 'chain' (every join under a chain of
    two single-child nodes)."""
    leaf = [lab + ":" + _length(rnd, zero) for lab in labs]
    if shape == "star":
        return "(" + ",".join(leaf) + ");"
    if shape == "caterpillar":
        if len(leaf) < 3:
            return "(" + ",".join(leaf) + ");"
        opens = "".join("(" + x + "," for x in leaf[:-2])
        closes = "".join("):" + _length(rnd, zero) for _ in leaf[:-3]) + ")"          # the outermost one is the root
        return opens + "(" + leaf[-2] + "," + leaf[-1] + "):" + _length(rnd, zero) + closes + ";"
    nodes = leaf
    while len(nodes) > 1:
        if shape == "balanced":
            nxt = []
            for k in range(0, len(nodes) - 1, 2):
                nxt.append("(" + nodes[k] + "," + nodes[k + 1] + ")" + (":" + _length(rnd, zero) if len(nodes) > 2 else ""))
            if len(nodes) % 2:
                nxt.append(nodes[-1])
            nodes = nxt
            continue
        k = min(len(nodes), rnd.choice((2, 2, 2, 3, 5)))
        at = rnd.randrange(len(nodes) - k + 1)
        joined = "(" + ",".join(nodes[at:at + k]) + ")"
        if len(nodes) > k:
            joined += ":" + _length(rnd, zero)
            if shape == "chain" or rnd.random() < 0.15:
                joined = "((" + joined + "):" + _length(rnd, zero) + "):" + _length(rnd, zero)
        nodes[at:at + k] = [joined]
    return nodes[0] + ";"


def forest(seed, specs):
    """specs: [(name, shape, nleaves, ngenomes, copies, zero[, prefix])] -> [(name, text)]"""
    rnd = random.Random(seed)
    return [(s[0], newick(s[1], labels(s[2], s[3], rnd, s[4], *s[6:7]), rnd, s[5])) for s in specs]


def golden_metadata(case):
    return {row[0]: {"taxonomy": row[1:8]} for row in case["metadata"]}


def check_golden_case(gt, case, d):
    """Runs paralogTest and consistencyTest of `gt` (a GeneTrees) on a case of tests/golden/genetrees_cases.json under the directory d and
    compares records, files and copied sets byte for byte.  Returns the infos of the two calls."""
    tree_dir, info_dir, clans = os.path.join(d, "trees"), os.path.join(d, "tigrfam_info"), os.path.join(d, "Pfam-A.clans.tsv")
    os.makedirs(tree_dir)
    os.makedirs(info_dir)
    for name, text in case["trees"].items():
        open(os.path.join(tree_dir, name), "w").write(text)
    for name, text in case["tigrfam_info"].items():
        open(os.path.join(info_dir, name), "w").write(text)
    open(clans, "w").write(case["pfam_clans"])
    md, expected, infos = golden_metadata(case), case["expected"], []
    if expected["paralog"] is not None:
        out = os.path.join(d, "conspecific")
        os.makedirs(out)
        open(os.path.join(out, "stale.tre"), "w").write("(a,b);\n")          # the output directory is emptied first
        records = gt.paralogTest(tree_dir, md, case["acceptPer"], case["extension"], out)
        assert records == expected["paralog"]["records"]
        assert sorted(os.listdir(out)) == expected["paralog"]["copied"]
        for f in expected["paralog"]["copied"]:
            assert open(os.path.join(out, f)).read() == case["trees"][f]
        infos.append(gt.lastInfo)
    desc = gt.readDescriptions(info_dir, clans)
    out, table = os.path.join(d, "final"), os.path.join(d, "consistency.tsv")
    os.makedirs(out)
    open(os.path.join(out, "stale.tre"), "w").write("(a,b);\n")
    results = gt.consistencyTest(tree_dir, md, desc, case["consistencyThreshold"], case["minTaxaForAverage"], case["extension"], table, out)
    want = expected["consistency"]
    assert sorted(os.listdir(os.path.join(out, "consistency"))) == sorted(want["results"])
    for f, text in want["results"].items():
        assert open(os.path.join(out, "consistency", f)).read() == text, f
    assert open(table).read() == want["table"]
    assert sorted(f for f in os.listdir(out) if os.path.isfile(os.path.join(out, f))) == want["copied"]
    assert sorted(results) == sorted(f for f in case["trees"] if f.endswith(case["extension"]))
    infos.append(gt.lastInfo)
    return infos
