"""Tetranucleotide signatures on the MI355X (checkm/genomicSignatures.py): the file `checkm tetra` writes and outliers, tetra_plot,
dist_plot and binTools read.

calculate() reads the FASTA file with the rules of CheckM's readFasta (ckm_nucseq_read), counts the canonical 4-mers of every sequence
on the device (ckm_nucstats_run) and writes the frequencies in file order, each formatted as str(numpy.float64) formats it.  There is
no CPU path for the file pass: without a device calculate() logs an error and exits.
"""
import logging
import sys

import numpy as np

from checkm_amd import _lib

_COMPL = str.maketrans('ACGT', 'TGCA')


def _rev_comp(seq):
    return seq.translate(_COMPL)[::-1]


def format_rows(ids, counts):
    """The rows of calculate()'s file for sequence ids and their [n, 136] canonical 4-mer counts: each count divided by the row's total
    as float64 (nan for a row without a valid window), formatted as str(numpy.float64) does -- the shortest repr of the float."""
    total = counts.sum(axis=1, dtype=np.uint64).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        freq = counts.astype(np.float64) / total[:, None]
    out = []
    for a in range(0, len(ids), 4096):
        rows = freq[a:a + 4096].tolist()
        out.append(''.join(ids[a + i] + '\t' + '\t'.join(map(repr, row)) + '\n' for i, row in enumerate(rows)))
    return ''.join(out)


class GenomicSignatures(object):
    def __init__(self, K, threads):
        self.logger = logging.getLogger('timestamp')
        self.K = K
        self.totalThreads = threads
        self.kmerCols, self.kmerToCanonicalIndex = self._makeKmerColNames()
        self.last_timing = {}

    def _makeKmerColNames(self):
        """Canonical k-mers (the lexicographically smaller of a k-mer and its reverse complement) in increasing order, and the column of
        every k-mer."""
        mers = ['']
        for _ in range(self.K):
            mers = [m + b for m in mers for b in 'ACGT']
        cols = sorted(set(min(m, _rev_comp(m)) for m in mers))
        index = {}
        for i, m in enumerate(cols):
            index[m] = i
            index[_rev_comp(m)] = i
        return cols, index

    def canonicalKmerOrder(self):
        return self.kmerCols

    def seqSignature(self, seq):
        """Frequencies of the canonical k-mers of seq (windows with anything but A/C/G/T after upper-casing are skipped)."""
        sig = [0] * len(self.kmerCols)
        s = seq.upper()
        for i in range(len(s) - self.K + 1):
            k = self.kmerToCanonicalIndex.get(s[i:i + self.K])
            if k is not None:
                sig[k] += 1
        sig = np.array(sig, dtype=float)
        with np.errstate(invalid='ignore'):
            sig /= np.sum(sig)
        return sig

    def calculate(self, seqFile, outputFile):
        """Write outputFile: a header (`Sequence Id` and the 136 tetranucleotides) and one row per sequence of seqFile, in file order."""
        import time
        from checkm_amd import runtime
        self.logger.info('Determining tetranucleotide signature of each sequence.')
        if self.K != 4:
            self.logger.error('The device pass counts tetranucleotides only (K = 4), not K = %d.' % self.K)
            sys.exit(1)
        try:
            ctx = runtime.get_ctx()
        except Exception as e:
            self.logger.error("No usable MI355X (gfx950) device for the tetranucleotide signatures: %s" % e)
            sys.exit(1)
        t0 = time.perf_counter()
        seqs = _lib.NucSeqs([seqFile])
        try:
            t1 = time.perf_counter()
            r = _lib.nucstats(ctx, seqs, tetra=True)
            t2 = time.perf_counter()
            ids = seqs.ids()
        finally:
            seqs.close()
        with open(outputFile, 'w') as fout:
            fout.write('Sequence Id')
            for kmer in self.canonicalKmerOrder():
                fout.write('\t' + kmer)
            fout.write('\n')
            fout.write(format_rows(ids, r['tetra']))
        t3 = time.perf_counter()
        self.last_timing = dict(read=t1 - t0, upload=r['ms_upload'] / 1e3, kernel=(r['ms_count'] + r['ms_fill']) / 1e3,
                                host=(t2 - t1) - (r['ms_upload'] + r['ms_count'] + r['ms_fill']) / 1e3, write=t3 - t2, bytes=r['bytes'])

    def distance(self, sig1, sig2):
        return np.sum(np.abs(sig1 - sig2))

    def read(self, tetraProfileFile):
        """{sequence id: frequencies} of a file written by calculate()."""
        sig = {}
        with open(tetraProfileFile) as f:
            next(f)
            for line in f:
                cols = line.split('\t')
                sig[cols[0]] = np.array([float(x) for x in cols[1:]])
        return sig
