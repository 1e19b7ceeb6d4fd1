#!/usr/bin/env python
"""Goldens of the per-window numbers of `checkm gc_plot`, `gc_bias_plot`, `coding_plot` and `tetra_plot` produced by the REFERENCE's own
plot classes (checkm/plot/*.py imported from a CheckM source tree named by CHECKM_SOURCE; matplotlib is needed for their base class):
plotOnAxes runs with recording stand-ins for the axes, and what reaches `hist` and `scatter` is captured -- the data lists, the
sequence lengths, the per-sequence distances; for gc_bias_plot the window and sequence GC behind the two scatter calls.  Failures are
recorded by type and args.  Fabricated reference distributions as in tools/gen_outliers_golden.py.

Only data is recorded: input texts, window sizes, the captured lists (every float as float.hex()).  The tetranucleotide profile rows are
not stored: the tests rebuild them with the restatement and compare their SHA-256.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_seqwin_golden.py > tests/golden/seqwin_cases.json
       CHECKM_SOURCE=<checkm source> python tools/gen_seqwin_golden.py --time --mb N     (times the reference's TD window loop on one core,
                                                                                          writes profiles/r13_seqwin_reference_cpu.json)"""
import hashlib
import json
import logging
import os
import random
import sys
import tempfile
import time
import warnings
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.gen_outliers_golden import DATA, MODEL, distributions, fasta, rnd  # noqa: E402  (sets CHECKM_DATA_PATH)

SMALL_W = [1, 3, 4, 5, 7]


class Options(object):
    font_size, dpi, width, height = 8, 72, 6.5, 3.5
    gc_window_size = cd_window_size = td_window_size = window_size = 5000
    gc_bin_width = cd_bin_width = td_bin_width = 0.01
    results_dir = None


def sprinkle(r, s, chars, n):
    s = list(s)
    for _ in range(n):
        s[r.randrange(len(s))] = r.choice(chars)
    return "".join(s)


def gene_rows(cid, spans):
    return "".join("%s\tProdigal_v2.6.3\tCDS\t%d\t%d\t10.0\t+\t0\tID=1_%d;partial=00\n" % (cid, a, z, k + 1) for k, (a, z) in enumerate(spans))


def build_cases():
    r = random.Random(20261018)
    cases = []
    # every length around the small windows from 4 up (a shorter sequence has a nan profile row and makes every distance nan); lower case, U / u, scattered N: no window without a base, so all four plots succeed
    plain = [("p%02d" % n, rnd(r, n)) for n in (4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 29)]
    plain += [("lower", rnd(r, 40).lower()), ("rna", rnd(r, 43).replace("T", "U")), ("mixed", sprinkle(r, rnd(r, 64), "Uun", 9).replace("n", "N")),
              ("seam_n", "ACGNACGTNCGTACGUACGTAUGTACGTACG"), ("long", sprinkle(r, rnd(r, 131), "acgtRY", 30))]
    gff = "##gff-version  3\n" + MODEL + gene_rows("p29", [(2, 9), (5, 7), (8, 20), (26, 28)]) + gene_rows("lower", [(1, 40)]) + \
        gene_rows("long", [(3, 30), (10, 20), (25, 60), (90, 100)]) + gene_rows("mixed", [(6, 7)]) + gene_rows("p14", [(1, 3)])
    cases.append(dict(name="plain", fasta=fasta(plain), gff=gff, windows=SMALL_W, profile_missing=[]))
    # what the reference trips over: an empty sequence, runs of N over whole windows
    edges = [("e_ok", rnd(r, 50)), ("e_nrun", rnd(r, 9) + "N" * 15 + rnd(r, 12)), ("e_empty", ""), ("e_alln", "N" * 17), ("e_tail", rnd(r, 22))]
    cases.append(dict(name="edges", fasta=">e_ok\n%s\n>e_nrun\n%s\n>e_empty\n>e_alln\n%s\n>e_tail\n%s\n>e1\nA\n>e2\nac\n>e3\nACG\n" % (edges[0][1], edges[1][1], edges[3][1], edges[4][1]),
                      gff="##gff-version  3\n" + MODEL + gene_rows("e_ok", [(1, 30)]) + gene_rows("e_nrun", [(5, 33)]), windows=SMALL_W, profile_missing=[]))
    big = [("b5000", rnd(r, 5000)), ("b5001", rnd(r, 5001)), ("b10000", rnd(r, 10000).lower()), ("b10001", sprinkle(r, rnd(r, 10001), "NUu", 300)),
           ("b12k", rnd(r, 4990) + "ACGT" * 5 + rnd(r, 6990))]
    cases.append(dict(name="big", fasta=fasta(big), gff="##gff-version  3\n" + MODEL + gene_rows("b10001", [(100, 900), (800, 5100), (4000, 4500), (9000, 9900)]) +
                      gene_rows("b12k", [(4900, 5100)]), windows=[5000], profile_missing=[]))
    bign = [("n_ok", rnd(r, 6000)), ("b1", "G"), ("n_run", rnd(r, 3000) + "N" * 10000 + rnd(r, 3000))]
    cases.append(dict(name="big_nrun", fasta=fasta(bign), gff="##gff-version  3\n" + MODEL + gene_rows("n_run", [(1, 2000)]), windows=[5000], profile_missing=[]))
    cases.append(dict(name="nogff", fasta=fasta([("g0", rnd(r, 30))]), gff=None, windows=[7], profile_missing=[]))
    cases.append(dict(name="missing_id", fasta=fasta([("k0", rnd(r, 30)), ("stranger", rnd(r, 25))]), gff="##gff-version  3\n" + MODEL, windows=[5], profile_missing=["stranger"]))
    cases.append(dict(name="short", fasta=fasta([("s0", rnd(r, 7)), ("s1", rnd(r, 3))]), gff="##gff-version  3\n" + MODEL + gene_rows("s0", [(1, 6)]), windows=[7, 5000],
                      profile_missing=[]))
    return cases


def axes():
    ax = mock.MagicMock()
    ax.get_ylim.return_value = (0.0, 1.0)
    ax.get_xlim.return_value = (0.0, 1.0)
    ax.get_yticks.return_value = [0.0, 1.0]
    return ax


def hexes(values):
    return [float(v).hex() for v in values]


def capture(fn, cap):
    """Runs fn; returns the failure (type and args) or None."""
    del cap.text[:]
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn()
    except SystemExit as e:
        return dict(type="SystemExit", code=e.code, log=list(cap.text))
    except (KeyError, ZeroDivisionError) as e:
        return dict(type=type(e).__name__, args=[str(a) for a in e.args])
    return None


def hist_scatter(plotter, args):
    """What one two-axes plot handed to hist (data) and to scatter (its x and y)."""
    a, b = axes(), axes()
    out = dict(error=None, data=None, seqLens=None, deltas=None)
    out["error"] = capture(lambda: plotter.plotOnAxes(*(args + [a, b])), CAP)
    if a.hist.called:
        out["data"] = hexes(a.hist.call_args[0][0])
    elif out["error"] is None:
        out["data"] = []                                            # the '[Error] No seqs >= ...' label: nothing was plotted
    if b.scatter.called:
        out["deltas"] = hexes(b.scatter.call_args[0][0])
        out["seqLens"] = [int(x) for x in b.scatter.call_args[0][1]]
    return out


class Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.text = []

    def emit(self, record):
        self.text.append(record.getMessage())


CAP = Capture()


def main():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    dist = distributions()
    for k, v in dist.items():
        open(os.path.join(DATA, "distributions", k + ".txt"), "w").write(v)
    from checkm.genomicSignatures import GenomicSignatures
    from checkm.plot.codingDensityPlots import CodingDensityPlots
    from checkm.plot.gcBiasPlots import GcBiasPlot
    from checkm.plot.gcPlots import GcPlots
    from checkm.plot.tetraDistPlots import TetraDistPlots
    from checkm.util.seqUtils import readFasta
    logging.getLogger("timestamp").addHandler(CAP)
    if "--time" in sys.argv:
        return time_reference(GenomicSignatures, int(sys.argv[sys.argv.index("--mb") + 1]))
    work = tempfile.mkdtemp(prefix="ckm_seqwin_gold_")
    result = dict(distributions=dist, cases=[])
    seen = set()
    for c in build_cases():
        d = os.path.join(work, c["name"])
        os.makedirs(os.path.join(d, "out", "bins", c["name"]))
        path = os.path.join(d, c["name"] + ".fna")
        open(path, "w").write(c["fasta"])
        if c["gff"] is not None:
            open(os.path.join(d, "out", "bins", c["name"], "genes.gff"), "w").write(c["gff"])
        seqs = readFasta(path)
        gs = GenomicSignatures(4, 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sigs = {k: gs.seqSignature(s) for k, s in seqs.items() if k not in c["profile_missing"]}
        c["profile_sha256"] = hashlib.sha256("".join(k + "".join(hexes(v)) for k, v in sigs.items()).encode()).hexdigest()
        c["runs"] = []
        for w in c["windows"]:
            o = Options()
            o.gc_window_size = o.cd_window_size = o.td_window_size = o.window_size = w
            o.results_dir = os.path.join(d, "out")
            run = dict(windowSize=w)
            run["gc_plot"] = hist_scatter(GcPlots(o), [path, [95]])
            run["coding_plot"] = hist_scatter(CodingDensityPlots(o), [path, [95]])
            run["tetra_plot"] = hist_scatter(TetraDistPlots(o), [path, sigs, [95]])
            cov = {k: [1.0, [1.0] * (max(0, (len(s) - 1) // w) if len(s) else 0)] for k, s in seqs.items()}
            a, b = axes(), axes()
            g = dict(error=capture(lambda: GcBiasPlot(o).plotOnAxes(path, cov, a, b), CAP), windowGC=None, seqGC=None)
            if a.scatter.called:
                g["windowGC"] = hexes(a.scatter.call_args[0][0])
            if b.scatter.called:
                g["seqGC"] = hexes(b.scatter.call_args[0][0])
            run["gc_bias_plot"] = g
            c["runs"].append(run)
            for p in ("gc_plot", "coding_plot", "tetra_plot", "gc_bias_plot"):
                seen.add((p, (run[p]["error"] or {}).get("type")))
                if p == "tetra_plot" and run[p]["data"] and "nan" in run[p]["data"]:
                    seen.add("nan" if len(set(run[p]["data"])) > 2 else "all nan")
        result["cases"].append(c)
    # the fixture cannot degenerate: every kind of outcome is there
    for need in (("gc_plot", None), ("coding_plot", None), ("tetra_plot", None), ("gc_bias_plot", None), ("coding_plot", "ZeroDivisionError"),
                 ("gc_bias_plot", "ZeroDivisionError"), ("coding_plot", "SystemExit"), ("tetra_plot", "KeyError"), "nan"):
        assert need in seen, (need, sorted(map(str, seen)))
    json.dump(result, sys.stdout, indent=0, ensure_ascii=True)
    sys.stdout.write("\n")


def time_reference(GenomicSignatures, mb):
    """The TD window loop of tetraDistPlots.py:63-79 on one core: seqSignature of every 5000-base window and its distance."""
    import numpy as np
    r = random.Random(1)
    seq = "".join(r.choice("ACGT") for _ in range(mb << 20))
    gs = GenomicSignatures(4, 1)
    binSig = gs.seqSignature(seq[:100000])
    t0 = time.perf_counter()
    start, end, n = 0, 5000, 0
    while end < len(seq):
        gs.distance(gs.seqSignature(seq[start:end]), binSig)
        start = end
        end += 5000
        n += 1
    dt = time.perf_counter() - t0
    out = dict(what="reference TD window loop (seqSignature + distance per window), one core", megabytes=mb, window=5000, windows=n, seconds=dt,
               seconds_per_256MB=dt * 256.0 / mb, numpy=np.__version__)
    open(os.path.join(ROOT, "profiles", "r13_seqwin_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
