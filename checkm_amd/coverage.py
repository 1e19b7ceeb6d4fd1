"""`checkm coverage` (checkm/coverage.py): coverage and mapped reads of every sequence under every BAM file.

The reference opens each BAM with pysam in worker processes, walks every read in Python and sends per-reference tuples through
queues.  Here the library reads the BAM itself (ckm_bam_open: BGZF blocks inflated on the host threads, no pysam, no index read) and
the records are classified on the device, a lane per record, with the reference's elif chain (ckm_coverage_run;
checkm_amd/csrc/coverage_dev.h).  What comes back is nine integers per reference sequence; the division, the file and the printed
read summary are done here, in the reference's formats.

Row order of the coverage file: the reference's order with one thread, for any number of threads -- the bins' sequences in binFiles
and FASTA order, then the BAM references that no bin holds in header order, per BAM in argument order."""
import logging
import ntpath
import os
import sys
import time
from collections import defaultdict

import numpy as np
from numpy import mean, sqrt

from checkm_amd import _lib, runtime
from checkm_amd.common import binIdFromFilename
from checkm_amd.defaultValues import DefaultValues


class CoverageStruct():
    def __init__(self, seqLen, mappedReads, coverage):
        self.seqLen = seqLen
        self.mappedReads = mappedReads
        self.coverage = coverage


SUMMARY_ROWS = (('properly mapped reads', 7), ('duplicate reads', 1), ('secondary reads', 2), ('reads failing QC', 3),
                ('reads failing alignment length', 4), ('reads failing edit distance', 5), ('reads not properly paired', 6))


def read_summary(totals):
    """The lines the reference prints after a BAM file (coverage.py:278-287) from the nine column sums, '' without reads (the reference
    divides by zero there)."""
    reads = int(totals[0])
    if reads == 0:
        return ''
    out = ['', '    # total reads: %d' % reads]
    for label, k in SUMMARY_ROWS:
        out.append('      # %s: %d (%.1f%%)' % (label, int(totals[k]), float(int(totals[k])) * 100 / reads))
    out.append('')
    return '\n'.join(out) + '\n'


def bin_sequences(binFiles):
    """({seqId: binId}, {seqId: length in code points}) over the bins in order, a later bin overwriting an earlier one (coverage.py:63-71)."""
    seqIdToBinId, seqIdToSeqLen = {}, {}
    if not binFiles:
        return seqIdToBinId, seqIdToSeqLen
    batch = _lib.NucSeqs(list(binFiles))
    try:
        ids = batch.ids()
        for f, binFile in enumerate(binFiles):
            binId = binIdFromFilename(binFile)
            for k in range(int(batch.file_first[f]), int(batch.file_first[f + 1])):
                raw = np.frombuffer(batch.seq(k), dtype=np.uint8)
                seqIdToBinId[ids[k]] = binId
                seqIdToSeqLen[ids[k]] = int(np.count_nonzero((raw & 0xC0) != 0x80))      # code points of the UTF-8 text
    finally:
        batch.close()
    return seqIdToBinId, seqIdToSeqLen


def coverage_text(bamFiles, seqIdToBinId, seqIdToSeqLen, coverageInfo):
    """The coverage file (coverage.py:97-119).  seqIdToSeqLen is updated with the BAM files' lengths as the reference does."""
    lines = ['Sequence Id\tBin Id\tSequence length (bp)' + '\tBam Id\tCoverage\tMapped reads' * len(bamFiles)]
    for bamFile in coverageInfo:
        for seqId, st in coverageInfo[bamFile].items():
            seqIdToSeqLen[seqId] = st.seqLen
    for seqId, seqLen in seqIdToSeqLen.items():
        row = seqId + '\t' + seqIdToBinId.get(seqId, DefaultValues.UNBINNED) + '\t' + str(seqLen)
        for bamFile in bamFiles:
            st = coverageInfo[bamFile].get(seqId)
            row += '\t%s\t%f\t%d' % ((binIdFromFilename(bamFile), st.coverage, st.mappedReads) if st is not None else (binIdFromFilename(bamFile), 0, 0))
        lines.append(row)
    return '\n'.join(lines) + '\n'


def structs_from_counters(references, lengths, counters):
    """{seqId: CoverageStruct} in header order; a reference of length 0 is the reference's ZeroDivisionError (coverage.py:232)."""
    info = {}
    for k, (seqId, seqLen) in enumerate(zip(references, lengths)):
        info[seqId] = CoverageStruct(seqLen=seqLen, mappedReads=int(counters[k][7]), coverage=float(int(counters[k][8])) / seqLen)
    return info


class Coverage():
    """Calculate coverage of all sequences."""

    def __init__(self, threads):
        self.logger = logging.getLogger('timestamp')
        self.totalThreads = threads
        self.last_timing = {}

    def _counters(self, bamFile, bAllReads, minAlignPer, maxEditDistPer, minQC):
        """(references, lengths, [n_ref, 9] counters, timing) of one BAM file: the device pass."""
        bam = _lib.Bam(bamFile)
        try:
            counters, timing = _lib.coverage_counters(runtime.get_ctx(), bam, bAllReads, minAlignPer, maxEditDistPer, minQC)
            return bam.references, bam.lengths, counters, timing
        except _lib.CoverageRecordError as e:
            if e.reason == 2:
                raise KeyError("tag 'NM' not present", "read '%s' (record %d of %s)" % (e.read, e.record, bamFile))
            raise
        finally:
            bam.close()

    def run(self, binFiles, bamFiles, outFile, bAllReads, minAlignPer, maxEditDistPer, minQC):
        """Calculate coverage of sequences for each BAM file."""
        t0 = time.perf_counter()
        self.logger.info('Determining bin assignment of each sequence.')
        seqIdToBinId, seqIdToSeqLen = bin_sequences(binFiles)
        t1 = time.perf_counter()

        self.logger.info("Processing %d file(s) with %d threads.\n" % (len(bamFiles), self.totalThreads))

        # make sure all BAM files are sorted
        self.numFiles = len(bamFiles)
        for bamFile in bamFiles:
            if not os.path.exists(bamFile + '.bai'):
                self.logger.error('BAM file is either unsorted or not indexed: ' + bamFile + '\n')
                sys.exit(1)

        coverageInfo = {}
        split = defaultdict(float)
        for k, bamFile in enumerate(bamFiles):
            self.logger.info('Processing %s (%d of %d):' % (ntpath.basename(bamFile), k + 1, len(bamFiles)))
            references, lengths, counters, timing = self._counters(bamFile, bAllReads, minAlignPer, maxEditDistPer, minQC)
            for f, v in timing.items():
                split[f] += v
            coverageInfo[bamFile] = structs_from_counters(references, lengths, counters)
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

        self.logger.info('Writing coverage information to file.')
        text = coverage_text(bamFiles, seqIdToBinId, seqIdToSeqLen, coverageInfo)
        if outFile != '':
            try:
                fout = open(outFile, 'w')
            except Exception:
                self.logger.error("Error diverting stdout to file: " + outFile)
                sys.exit(1)
            with fout:
                fout.write(text)
        else:
            sys.stdout.write(text)
        t3 = time.perf_counter()
        self.last_timing = dict(split, s_bins=t1 - t0, s_bams=t2 - t1, s_write=t3 - t2, s_total=t3 - t0, bams=len(bamFiles))

    def parseCoverage(self, coverageFile):
        """{binId: {seqId: {bamId: coverage}}} of a coverage file."""
        coverageStats = {}
        with open(coverageFile) as f:
            next(f, None)
            for line in f:
                lineSplit = line.split('\t')
                perSeq = coverageStats.setdefault(lineSplit[1], {}).setdefault(lineSplit[0], {})
                for i in range(3, len(lineSplit), 3):
                    perSeq[lineSplit[i]] = float(lineSplit[i + 1])
        return coverageStats

    def binProfiles(self, coverageFile):
        """{binId: {bamId: [mean coverage weighted by sequence length, standard deviation over the sequences]}} of a coverage file; the
        running mean and the variance are evaluated in the reference's order (coverage.py:315-358)."""
        binCoverages = defaultdict(lambda: defaultdict(list))
        binStats = defaultdict(dict)
        with open(coverageFile) as f:
            next(f, None)
            for line in f:
                lineSplit = line.split('\t')
                binId, seqLen = lineSplit[1], int(lineSplit[2])
                for i in range(3, len(lineSplit), 3):
                    bamId, coverage = lineSplit[i], float(lineSplit[i + 1])
                    binCoverages[binId][bamId].append(coverage)
                    prevLength, prevMean = binStats[binId].get(bamId, (0, 0))
                    binLength = prevLength + seqLen
                    weight = float(seqLen) / binLength
                    binStats[binId][bamId] = [binLength, coverage * weight + prevMean * (1 - weight)]

        profiles = defaultdict(dict)
        for binId in binStats:
            for bamId, (_binLength, meanBinCoverage) in binStats[binId].items():
                coverages = binCoverages[binId][bamId]
                varCoverage = 0
                if len(coverages) > 1:
                    varCoverage = mean([(x - meanBinCoverage) ** 2 for x in coverages])
                profiles[binId][bamId] = [meanBinCoverage, sqrt(varCoverage)]
        return profiles
