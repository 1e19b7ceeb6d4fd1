"""CoverageWindows of `checkm gc_bias_plot` (checkm/coverageWindows.py): coverage of every reference sequence of a BAM file and of its
windows.

The reference allocates a float64 depth array of every reference's length, adds 1.0 to a slice of it per read in Python through pysam
callbacks and sums the array window by window with Python's sum.  Here the library reads the BAM itself (ckm_bam_open, no pysam) and
the device classifies every record with THIS file's chain -- which is not the chain of `checkm coverage` -- and scatters every mapped
read into per-window accumulators with O(1) memory operations (ckm_coverage_windows_run; checkm_amd/csrc/covwin_dev.h).  What comes
back is nine integers per reference and one integer per window; each reported value is one float64 division of an exact integer, as
in the reference, whose sums of whole numbers below 2^53 are exact in any order."""
import logging
import ntpath
import os
import sys
import time

import numpy as np

from checkm_amd import _lib, runtime
from checkm_amd.coverage import CoverageStruct, read_summary          # noqa: F401  (CoverageStruct: the reference defines it here too)

NO_CIGAR = "'<' not supported between instances of 'NoneType' and 'float'"


def windows_from_sums(references, lengths, counters, first, sums, windowSize):
    """{seqId: [coverage, windowCoverages]} in header order.  Window k is reported while (k + 1) * w < L: a reference's last slot (its
    tail, or a window that ends exactly at L) is not.  A reference of length 0 is the reference's ZeroDivisionError."""
    info = {}
    w = np.float64(windowSize)
    for k, (seqId, seqLen) in enumerate(zip(references, lengths)):
        a, b = int(first[k]), int(first[k + 1])
        windowCoverages = (sums[a:max(a, b - 1)].astype(np.float64) / w).tolist()
        info[seqId] = [float(int(counters[k][8])) / seqLen, windowCoverages]
    return info


class CoverageWindows():
    """Calculate coverage of all sequences."""

    def __init__(self, threads):
        self.logger = logging.getLogger('timestamp')
        self.totalThreads = threads
        self.last_timing = {}

    def _pass(self, bamFile, bAllReads, minAlignPer, maxEditDistPer, windowSize):
        """(references, lengths, [n_ref, 9] counters, first slots, depth sums, timing) of the BAM file: the device pass."""
        bam = _lib.Bam(bamFile)
        try:
            counters, first, sums, timing = _lib.coverage_windows(runtime.get_ctx(), bam, bAllReads, minAlignPer, maxEditDistPer, windowSize)
            return bam.references, bam.lengths, counters, first, sums, timing
        finally:
            bam.close()

    def run(self, binFiles, bamFile, bAllReads, minAlignPer, maxEditDistPer, windowSize):
        """Calculate coverage of full sequences and windows."""
        t0 = time.perf_counter()

        # make sure BAM file is sorted
        if not os.path.exists(bamFile + '.bai'):
            self.logger.error('BAM file is not sorted: ' + bamFile + '\n')
            sys.exit(1)

        if windowSize != int(windowSize) or windowSize < 1:
            raise ValueError('windowSize must be a whole number of at least 1 (the reference never ends below that): %r' % (windowSize,))
        windowSize = int(windowSize)

        self.logger.info('Calculating coverage of windows.')
        try:
            references, lengths, counters, first, sums, timing = self._pass(bamFile, bAllReads, minAlignPer, maxEditDistPer, windowSize)
        except _lib.CoverageRecordError as e:
            where = "read '%s' (record %d of %s)" % (e.read, e.record, bamFile)
            if e.reason == 2:
                raise KeyError("tag 'NM' not present", where)
            if e.reason == 5:
                raise TypeError(NO_CIGAR, where)
            raise
        t1 = time.perf_counter()
        coverageInfo = windows_from_sums(references, lengths, counters, first, sums, windowSize)

        if self.logger.getEffectiveLevel() <= logging.INFO:
            n = len(references)
            if n:
                sys.stderr.write('    Finished processing %d of %d (%.2f%%) reference sequences.\r\n' % (n, n, 100.0))
                sys.stderr.flush()
            text = read_summary(counters.sum(axis=0) if n else [0] * 9)
            if text:
                sys.stdout.write(text)
            else:
                self.logger.warning('No reads in %s: no read summary.' % ntpath.basename(bamFile))
        t2 = time.perf_counter()
        self.last_timing = dict(timing, s_pass=t1 - t0, s_python=t2 - t1, s_total=t2 - t0)
        return coverageInfo
