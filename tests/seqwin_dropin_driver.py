"""TEST INFRASTRUCTURE: run in a process of its own by the drop-in tests of the plot hooks (a `checkm` package must not enter the test
process).  After dropin.install() the four plot classes run every golden case with recording axes; what reaches `hist` and `scatter`
must equal tests/golden/seqwin_cases.json, with one pass of the library per (file, window size) and no call answered by the ordinary
implementation.

usage: python tests/seqwin_dropin_driver.py emu|gpu <work dir> [<CheckM source tree>]
  emu: the device pass is the host executor (tests/emu/seqwin.py); gpu: the library's own.
  Without a source tree the plot classes are the project's own stand-ins (tests/seqwin_standin.py: a generic window walker over the
  hooked names).  That run covers the hook PROTOCOL only: the same names asked for the same windows must give the goldens' numbers.  The
  stand-ins have no drawing half, so what the reference meets there (the ZeroDivisionError of gc_plot inside BinTools.gcDist after its
  histogram, the log line in front of coding_plot's exit) is compared only when the reference's own, unmodified classes run, which
  needs a source tree."""
import json
import logging
import os
import sys
import warnings
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Options(object):
    font_size, dpi, width, height = 8, 72, 6.5, 3.5
    gc_bin_width = cd_bin_width = td_bin_width = 0.01


class Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.text = []

    def emit(self, record):
        self.text.append(record.getMessage())


def axes():
    ax = mock.MagicMock()
    ax.get_ylim.return_value = ax.get_xlim.return_value = (0.0, 1.0)
    ax.get_yticks.return_value = [0.0, 1.0]
    return ax


def hexes(values):
    return [float(v).hex() for v in values]


def run_plot(fn, cap):
    """(failure or None, first axes, second axes) of fn(first, second)."""
    a, b = axes(), axes()
    del cap.text[:]
    error = None
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn(a, b)
    except SystemExit as e:
        error = dict(type="SystemExit", code=e.code, log=list(cap.text))
    except (KeyError, ZeroDivisionError) as e:
        error = dict(type=type(e).__name__, args=[str(x) for x in e.args])
    return error, a, b


def main():
    mode, work = sys.argv[1], sys.argv[2]
    source = sys.argv[3] if len(sys.argv) > 3 else None
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "seqwin_cases.json")))
    if source:
        data = os.path.join(work, "data")                  # the reference wants a data root at import time and reads its distributions
        os.makedirs(os.path.join(data, "pfam"))
        os.makedirs(os.path.join(data, "distributions"))
        open(os.path.join(data, "pfam", "Pfam-A.hmm.dat"), "w").close()
        for k, v in gold["distributions"].items():
            open(os.path.join(data, "distributions", k + ".txt"), "w").write(v)
        os.environ["CHECKM_DATA_PATH"] = data
        sys.path.insert(0, source)
    else:
        from tests import seqwin_standin
        sys.path.insert(0, seqwin_standin.write_package(os.path.join(work, "stand_in")))
    import numpy as np
    from checkm.plot.codingDensityPlots import CodingDensityPlots
    from checkm.plot.gcBiasPlots import GcBiasPlot
    from checkm.plot.gcPlots import GcPlots
    from checkm.plot.tetraDistPlots import TetraDistPlots
    import checkm_amd.dropin
    checkm_amd.dropin.install()
    from checkm_amd import _lib, plotHooks, runtime
    from tests import seqwin_reference as ref
    if mode == "emu":
        from tests.emu import seqwin as emu
        runtime.get_ctx = lambda: None
        _lib.seq_windows = emu.seq_windows
    cap = Capture()
    logging.getLogger("timestamp").addHandler(cap)
    checked = 0
    for c in gold["cases"]:
        d = os.path.join(work, c["name"])
        os.makedirs(os.path.join(d, "out", "bins", c["name"]))
        path = os.path.join(d, c["name"] + ".fna")
        open(path, "w").write(c["fasta"])
        if c["gff"] is not None:
            open(os.path.join(d, "out", "bins", c["name"], "genes.gff"), "w").write(c["gff"])
        seqs = ref.read_fasta(c["fasta"])
        with np.errstate(invalid="ignore"):
            sigs = {k: ref.signature(s) for k, s in seqs.items() if k not in c["profile_missing"]}
        for run in c["runs"]:
            w = run["windowSize"]
            o = Options()
            o.gc_window_size = o.cd_window_size = o.td_window_size = o.window_size = w
            o.results_dir = os.path.join(d, "out")
            plotHooks.reset()
            tag = "%s w=%d " % (c["name"], w)
            for name, cls, args in (("gc_plot", GcPlots, [path, [95]]), ("coding_plot", CodingDensityPlots, [path, [95]]), ("tetra_plot", TetraDistPlots, [path, sigs, [95]])):
                want = run[name]
                error, a, b = run_plot(lambda x, y: cls(o).plotOnAxes(*(args + [x, y])), cap)
                if source:
                    assert error == want["error"], (tag + name, error, want["error"])
                elif name != "gc_plot":
                    strip = lambda e: e and {k: v for k, v in e.items() if k != "log"}
                    assert strip(error) == strip(want["error"]), (tag + name, error, want["error"])
                data = hexes(a.hist.call_args[0][0]) if a.hist.called else ([] if error is None else None)
                assert data == want["data"], (tag + name, data, want["data"])
                if b.scatter.called and want["seqLens"] is not None:
                    assert [int(x) for x in b.scatter.call_args[0][1]] == want["seqLens"], tag + name
                    if name == "tetra_plot":
                        assert hexes(b.scatter.call_args[0][0]) == want["deltas"], tag + name
                else:
                    assert want["seqLens"] is None or not want["data"], tag + name
                checked += 1
            want = run["gc_bias_plot"]
            cov = {k: [1.0, [1.0] * (max(0, (len(s) - 1) // w) if len(s) else 0)] for k, s in seqs.items()}
            error, a, b = run_plot(lambda x, y: GcBiasPlot(o).plotOnAxes(path, cov, x, y), cap)
            assert error == want["error"], (tag + "gc_bias_plot", error, want["error"])
            if error is None:
                assert hexes(a.scatter.call_args[0][0]) == want["windowGC"] and hexes(b.scatter.call_args[0][0]) == want["seqGC"], tag + "gc_bias_plot"
            checked += 1
            assert plotHooks.fallbacks == 0, (tag, plotHooks.fallbacks)
            # one pass for (file, w); a bin without a window is never asked about one, and gc_bias_plot's whole-sequence counts make the one pass
            assert plotHooks.library_calls == 1, (tag, plotHooks.library_calls)
    # off the grid and plain text: the ordinary implementation, counted
    plotHooks.reset()
    from checkm.plot import gcPlots
    seq = next(iter(gcPlots.readFasta(path).values()))
    assert gcPlots.baseCount(seq[1:4]) == ref.base_count(str(seq)[1:4]) and gcPlots.baseCount("ACGU") == (1, 1, 1, 1) and plotHooks.fallbacks == 2
    print("ok %d" % checked)


if __name__ == "__main__":
    main()
