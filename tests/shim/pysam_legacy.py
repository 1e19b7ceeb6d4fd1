"""TEST INFRASTRUCTURE -- the stand-in of tests/shim/pysam.py with the OLD pysam names that checkm/coverageWindows.py touches, so that
the REFERENCE's own CoverageWindows can run where pysam is not installed: tools/gen_covwin_golden.py binds `sys.modules['pysam']` and
`checkm.coverageWindows.pysam` to this module and records what the reference returns (tests/golden/covwin_cases.json).  Never imported
by checkm_amd.

What the reference relies on (checkm/coverageWindows.py:55-79, 118-120, 179-183), FROM MEMORY of pysam 0.2x like the rest of the shim
(DESIGN section 16 marks each with [pysam-ext]):
  read.rlen   = query_length = l_seq (0 for l_seq == 0)
  read.alen   = reference_length: the sum of the M, D, N, = and X lengths of the CIGAR, None for a record without CIGAR
  read.pos    = reference_start, 0-based
  read.opt(t) = get_tag(t)
  Samfile.fetch(ref, 0, len, callback=f) calls f for every record whose refID is ref, in file order, and returns nothing."""
from tests.shim import pysam as _base

M, D, N, EQ, X = 0, 2, 3, 7, 8


class AlignedSegment(_base.AlignedSegment):
    @property
    def rlen(self):
        return self.query_length

    @property
    def alen(self):
        if not self.cigar:
            return None
        return sum(n for op, n in self.cigar if op in (M, D, N, EQ, X))

    @property
    def pos(self):
        return self.reference_start

    def opt(self, tag):
        return self.get_tag(tag)


class Samfile(_base.Samfile):
    def __init__(self, path, mode="rb"):
        _base.Samfile.__init__(self, path, mode)
        for r in self._reads:
            r.__class__ = AlignedSegment

    def fetch(self, reference, start=None, end=None, callback=None):
        reads = _base.Samfile.fetch(self, reference, start, end)
        if callback is None:
            return reads
        for r in reads:
            callback(r)


AlignmentFile = Samfile
