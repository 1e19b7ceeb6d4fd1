#!/usr/bin/env python
"""Goldens of Unbinned: the reference's own checkm.unbinned.Unbinned().run over small hand-made bins and assemblies.  Per case the inputs,
both output files as they lie after the call (None: not created), the records of the 'timestamp' logger and a failure by type and
message.  Runs only where a CheckM source tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_unbinned_golden.py                 (writes tests/golden/unbinned_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_unbinned_golden.py --time --mb N   (times the reference's run on one core over the
                                                              assembly of tools/unbinned_bench.py, writes profiles/r15_unbinned_reference_cpu.json)"""
import gzip
import json
import locale
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A20 = "ACGTACGTACGTACGTACGT"


def case(name, bins, assembly, minSeqLen):
    return dict(name=name, bins=[dict(name=n, text=t) for n, t in bins], assembly=assembly, minSeqLen=minSeqLen)


def cases():
    c = []
    # an id in two bins (counted twice in the binned bases), a bin id absent from the assembly, lower case, U and N, blank lines, a header with a description
    c.append(case("basic", [("b1.fna", ">c1 first\nACGTAC\nGGTT\n\n>c2\nacgtacgtnn\n"), ("b2.fna", ">c2\nacgtacgtnn\n>ghost\nAAAAAAAAAAAA\n")],
                  ">c1 first\nACGTAC\nGGTT\n>c2 x\nacgtacgtnn\n\n>c3\nGGGCCCuuUUaaNNnn\n   \n>c4 desc here\nacgt\n>c5\nGCGCGCGCATNNNNNNNNNNxyz\n>c6\nAT\nGC\nGG\n", 5))
    # a repeated id whose later copy changes the length across minSeqLen, both ways; the id keeps its first place
    c.append(case("repeated", [("b1.fna", ">none\nACGT\n")],
                  ">up\nACGT\n>down\n" + A20 + "\n>mid\nGGGGGCCCCCAT\n>up\n" + A20 + "GG\n>down\nAC\n>tail\nTTTTTTTTTTTTG\n", 10))
    # only N: below minSeqLen it is skipped without error
    c.append(case("n_short", [], ">a\n" + A20 + "\n>n\nNNNNNNNN\n>b\nGGGGGGGGGGGGGGGGAAAA\n", 10))
    # only N at minSeqLen: the error, after its record, before its row; what follows is not written
    c.append(case("n_long", [("b1.fna", ">z\nAC\n")], ">a\n" + A20 + "\n>n\nNNNNNNNNNN\n>b\nGGGGGGGGGGGGGGGGAAAA\n", 10))
    # multi-byte UTF-8 in a sequence line: the length is in code points (u1 has 12 bytes and 9 code points; u2 has 10 and 10), and in an id
    c.append(case("utf8", [("b1.fna", ">binéd\nACGTACGTACGT\n")],
                  ">u1\nACGéé€TGC\n>u2\nACGTACGTAC\n>u3 é\nACéGTACG\U0001F9ECTACGTTTT\n>binéd\nACGTACGTACGT\n>éid\nGGGGGGGGGGGGC\n", 10))
    # no final newline: readFasta drops the last character of the file
    c.append(case("no_final_newline", [("b1.fna", ">c1\nACGTACGTAA")], ">c1\nACGTACGTAA\n>c2\nGGGGGGGGGGC\n>c3\nACGTACGTACG", 10))
    # a gzipped bin, CR LF and lone CR line ends
    c.append(case("gz_crlf", [("b1.fna.gz", ">c2\r\nGGGGCCCC\r\n"), ("b2.fna", ">c4\rAAAA\r")], ">c1\r\nACGTAC\r\nGT\r\n>c2\r\nGGGGCCCC\r\n>c3\rAAAAAAAT\rTT\r>c4\nAAAA\n", 4))
    # minSeqLen 0 keeps an empty sequence: the error at its row
    c.append(case("min0_empty", [], ">a\nACGT\n>empty\n>b\nGG\n", 0))
    # an empty assembly: both files complete, the error at the first percentage
    c.append(case("empty_assembly", [("b1.fna", ">c1\nACGT\n")], "", 0))
    # sequences but no base at all: the error at the second percentage
    c.append(case("no_base", [], ">e1\n>e2\n\n", 1))
    # every contig binned: a header-only stats file
    c.append(case("all_binned", [("b1.fna", ">c1\nACGTACGT\n>c2\nGGGG\n"), ("b2.fna", ">c3\nTTTTTTTT\n")], ">c1\nACGTACGT\n>c2\nGGGG\n>c3\nTTTTTTTT\n", 1))
    # rows whose GC lands on and next to a rounding tie of %.2f (1/8 = 12.5 %, 1/32 = 3.125 %, 3/32, 1/3, 2/3)
    c.append(case("ties", [], ">t8\nGAAAAAAA\n>t32\nC" + "A" * 31 + "\n>t96\nGCG" + "T" * 29 + "\n>t3\nGAT\n>t23\nGCT\n>t160\nG" + "A" * 159 + "\n", 1))
    # the missing assembly
    c.append(case("missing", [("b1.fna", ">c1\nACGT\n")], None, 1))
    return c


def write_inputs(d, c):
    """(bin paths, assembly path) of a case written under directory d, byte for byte."""
    paths = []
    for b in c["bins"]:
        p = os.path.join(d, b["name"])
        data = b["text"].encode("utf-8")
        if p.endswith(".gz"):
            with gzip.GzipFile(p, "wb", mtime=0) as g:
                g.write(data)
        else:
            open(p, "wb").write(data)
        paths.append(p)
    asm = os.path.join(d, "assembly.fna")
    if c["assembly"] is not None:
        open(asm, "wb").write(c["assembly"].encode("utf-8"))
    return paths, asm


class Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.out = []

    def emit(self, record):
        self.out.append([record.levelname, record.getMessage()])


def read_or_none(p):
    return open(p, "rb").read().decode("utf-8") if os.path.exists(p) else None


def run_case(Unbinned, c):
    d = tempfile.mkdtemp(prefix="ckm_unbinned_golden_")
    bins, asm = write_inputs(d, c)
    seqOut, statsOut = os.path.join(d, "out.fna"), os.path.join(d, "out.tsv")
    logger = logging.getLogger("timestamp")
    h = Records()
    logger.addHandler(h)
    logger.setLevel(logging.INFO)
    error = None
    try:
        Unbinned().run(bins, asm, seqOut, statsOut, c["minSeqLen"])
    except (Exception, SystemExit) as e:
        error = dict(type=type(e).__name__, message=str(e))
    finally:
        logger.removeHandler(h)
    # the failed call's frame is gone with its exception: its two files are closed as they are at interpreter exit
    log = [[lvl, m.replace(d + os.sep, "<dir>/")] for lvl, m in h.out]
    return dict(c, out_seq=read_or_none(seqOut), out_stats=read_or_none(statsOut), log=log, error=error)


def main():
    assert locale.getpreferredencoding(False).upper().replace("-", "") == "UTF8", "run under a UTF-8 locale (or python -X utf8): the reference opens its files with the default encoding"
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    from checkm.unbinned import Unbinned
    if "--time" in sys.argv:
        return time_reference(Unbinned, float(sys.argv[sys.argv.index("--mb") + 1]))
    out = dict(generator="tools/gen_unbinned_golden.py: checkm.unbinned.Unbinned().run of the reference; <dir>/ stands for the directory of the inputs",
               cases=[run_case(Unbinned, c) for c in cases()])
    open(os.path.join(ROOT, "tests", "golden", "unbinned_cases.json"), "w").write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for c in out["cases"]:
        print(c["name"], c["error"], len(c["log"]))


def time_reference(Unbinned, mb):
    from tools.unbinned_bench import synth_assembly
    d = tempfile.mkdtemp(prefix="ckm_unbinned_time_")
    bins, asm = synth_assembly(d, 20, mb, 5000)
    t0 = time.perf_counter()
    Unbinned().run(bins, asm, os.path.join(d, "out.fna"), os.path.join(d, "out.tsv"), 1000)
    wall = time.perf_counter() - t0
    out = dict(what="reference Unbinned.run, one core: 20 bins, minSeqLen 1000, the assembly of tools/unbinned_bench.py", megabytes=mb, seconds=wall,
               megabytes_per_second=mb / wall)
    open(os.path.join(ROOT, "profiles", "r15_unbinned_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
