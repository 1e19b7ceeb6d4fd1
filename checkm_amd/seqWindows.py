"""Per-window GC, coding density and tetranucleotide distance of a bin: the numbers `checkm gc_plot`, `gc_bias_plot`, `coding_plot`,
`tetra_plot` and `dist_plot` compute inline in their plot classes (checkm/plot/gcPlots.py:55-75, gcBiasPlots.py:51-66,
codingDensityPlots.py:73-89, tetraDistPlots.py:63-79).  The reference has no class for this; SequenceWindows returns exactly the lists
those loops build.

The file is read with the rules of CheckM's readFasta (ckm_nucseq_read); the base counts and the canonical 4-mers of every window are
counted on the device and the distance to the bin's signature is formed there in numpy's summation order (ckm_seq_windows_run); the
coding bases per window come from the merged intervals of the bin's genes.gff on the host (ckm_seq_windows_coding).  Every quotient is
one float64 division of integers, as in the reference.  There is no CPU path for the device pass.

Window k = [k w, (k + 1) w) exists while (k + 1) w < len(seq): the reference's `while end < seqLen`.

Declared differences: a windowSize below 1 or one that is no integer raises ValueError (the reference loops forever or fails inside a
slice).  A sequence with non-ASCII characters is not sent to the device: the Python statement below computes it (same result) and a
DEBUG line names it.
"""
import logging
import sys
import time

import numpy as np

from checkm_amd import _lib
from checkm_amd.defaultValues import DefaultValues


def _base_count(seq):
    s = seq.upper()
    return s.count('A'), s.count('C'), s.count('G'), s.count('T') + s.count('U')


def _check_window(windowSize):
    if isinstance(windowSize, bool) or not isinstance(windowSize, (int, np.integer)) or windowSize < 1 or windowSize > 2 ** 31 - 1:
        raise ValueError('windowSize must be an integer between 1 and 2^31 - 1, not %r' % (windowSize,))
    return int(windowSize)


class SequenceWindows(object):
    """The per-window passes of the plot commands."""

    def __init__(self, threads=1):
        """threads is accepted for the signature of CheckM's classes and not used: the library sizes its own host threads."""
        self.logger = logging.getLogger('timestamp')
        self.last_timing = {}

    # ---- the device pass ---------------------------------------------------------------------------------------------------------------

    def _run(self, fastaFile, windowSize, binSigOf=None, gffFile=None, wantTetra=False, seqs=None):
        """ids, lens, first, base [nwin, 4], seq [nseq, 4], td [nwin] or None, coding [nwin] or None of one file.  seqs: the file as an
        open _lib.NucSeqs batch, which stays the caller's; without it the file is read and the batch closed here."""
        from checkm_amd import runtime
        w = _check_window(windowSize)
        try:
            ctx = runtime.get_ctx()
        except Exception as e:
            self.logger.error("No usable MI355X (gfx950) device for the sequence windows: %s" % e)
            sys.exit(1)
        t0 = time.perf_counter()
        own = seqs is None
        if own:
            seqs = _lib.NucSeqs([fastaFile])
        try:
            t1 = time.perf_counter()
            ids = seqs.ids()
            # len(seq) of every sequence without decoding it: a sequence of L > 0 code points has L - 1 windows of one
            lens = _lib.seq_lengths(seqs)
            binSig = None
            if binSigOf is not None:
                binSig = binSigOf(ids, lens)
            sig = None if binSig is None else np.asarray(binSig, dtype=np.float64).reshape(1, 136)
            try:
                r = _lib.seq_windows(ctx, seqs, w, bin_sig=sig, want_tetra=wantTetra)
            except _lib.CkmError as e:
                if not wantTetra or e.code != -7:
                    raise
                wantTetra = False                                  # the 136 counts of every window do not fit the budget
                r = _lib.seq_windows(ctx, seqs, w, bin_sig=sig)
            t2 = time.perf_counter()
            coding = None
            if gffFile is not None:
                coding, _missing = _lib.seq_windows_coding(seqs, [gffFile], w)
            t3 = time.perf_counter()
            first = [int(x) for x in r['first']]
            base, per_seq, td = r['base'].astype(np.int64), r['seq'].astype(np.int64), r['td']
            tetra = r['tetra']
            for s in range(seqs.nseq):
                if not r['skipped'][s]:
                    continue
                # non-ASCII: the reference's own statement, window by window
                self.logger.debug('Sequence %s holds non-ASCII characters: its windows are computed on the host.' % ids[s])
                seq = seqs.seq(s).decode('utf-8')
                per_seq[s] = _base_count(seq)
                for k in range(first[s + 1] - first[s]):
                    win = seq[k * w:(k + 1) * w]
                    base[first[s] + k] = _base_count(win)
                    if tetra is not None:
                        from checkm_amd.genomicSignatures import GenomicSignatures
                        index = GenomicSignatures(4, 1).kmerToCanonicalIndex
                        u = win.upper()
                        for i in range(len(u) - 3):
                            c = index.get(u[i:i + 4])
                            if c is not None:
                                tetra[first[s] + k, c] += 1
                    if td is not None:
                        from checkm_amd.genomicSignatures import GenomicSignatures
                        gs = GenomicSignatures(4, 1)
                        td[first[s] + k] = gs.distance(gs.seqSignature(win), binSig)
        finally:
            if own:
                seqs.close()
        t4 = time.perf_counter()
        dev = (r['ms_upload'] + r['ms_count'] + r['ms_td'] + r['ms_download']) / 1e3
        self.last_timing = dict(read=t1 - t0, copy_in=r['ms_upload'] / 1e3, count=r['ms_count'] / 1e3, td=r['ms_td'] / 1e3, copy_out=r['ms_download'] / 1e3,
                                coding=t3 - t2, python=(t2 - t1) - dev + (t4 - t3), windows=int(r['windows']), pieces=int(r['pieces']), batches=int(r['batches']),
                                bytes=int(r['bytes']), skipped=int(r['skipped_seqs']))
        return dict(ids=ids, lens=lens, first=first, base=base, seq=per_seq, td=td, coding=coding, binSig=binSig, tetra=tetra, skipped=r['skipped'])

    def _done(self, t0):
        self.last_timing['python'] += time.perf_counter() - t0

    # ---- the lists of the plot classes -------------------------------------------------------------------------------------------------

    def gcWindows(self, fastaFile, windowSize):
        """(data, seqLens) of GcPlots.plotOnAxes: GC of every window with an A, C, G, T or U (the others are left out), len of every sequence."""
        r = self._run(fastaFile, windowSize)
        t0 = time.perf_counter()
        b = r['base']
        gc, den = (b[:, 2] + b[:, 1]).tolist(), b.sum(axis=1).tolist()
        data = [float(n) / d for n, d in zip(gc, den) if d]
        self._done(t0)
        return data, r['lens']

    def gcProfile(self, binFile, windowSize):
        """{seqId: [seqGC, windowGCs]} of GcBiasPlot.plotOnAxes; ZeroDivisionError where the reference raises it."""
        r = self._run(binFile, windowSize)
        t0 = time.perf_counter()
        b, q, first = r['base'], r['seq'], r['first']
        gc, den = (b[:, 2] + b[:, 1]).tolist(), b.sum(axis=1).tolist()
        profile = {}
        for s, seqId in enumerate(r['ids']):
            windowGCs = [float(gc[x]) / den[x] for x in range(first[s], first[s + 1])]
            a, c, g, t = (int(v) for v in q[s])
            profile[seqId] = [float(g + c) / (a + c + g + t), windowGCs]
        self._done(t0)
        return profile

    def cdWindows(self, fastaFile, gffFile, windowSize):
        """(data, seqLens) of CodingDensityPlots.plotOnAxes: coding bases of every window over its A, C, G, T, U."""
        _check_window(windowSize)
        import os
        if not os.path.exists(gffFile):
            self.logger.error('Missing gene feature file (%s). This plot if not compatible with the --genes option.' % DefaultValues.PRODIGAL_GFF)
            sys.exit(1)
        r = self._run(fastaFile, windowSize, gffFile=gffFile)
        t0 = time.perf_counter()
        den = r['base'].sum(axis=1).tolist()
        data = [float(c) / d for c, d in zip(r['coding'].tolist(), den)]
        self._done(t0)
        return data, r['lens']

    def tdWindows(self, fastaFile, tetraSigs, windowSize):
        """(data, seqLens, deltaTDs) of TetraDistPlots.plotOnAxes: Manhattan distance of every window's signature (nan for a window
        without a tetranucleotide) and of every sequence's profile row to the bin's signature."""
        def binSigOf(ids, lens):
            # BinTools.binTetraSig: every row times its weight, added in file order; KeyError for an id the profile does not hold
            binSize = sum(lens)
            sig = None
            for seqId, n in zip(ids, lens):
                weighted = tetraSigs[seqId] * (float(n) / binSize)
                if sig is None:
                    sig = weighted
                else:
                    sig += weighted
            if sig is None:                                        # a file without sequences: the reference's binTetraSig returns a name it never bound
                raise UnboundLocalError("cannot access local variable 'binSig' where it is not associated with a value")
            return sig
        r = self._run(fastaFile, windowSize, binSigOf=binSigOf)
        t0 = time.perf_counter()
        deltaTDs = [np.sum(np.abs(tetraSigs[seqId] - r['binSig'])) for seqId in r['ids']]
        data = [np.float64(x) for x in r['td'].tolist()]
        self._done(t0)
        return data, r['lens'], deltaTDs
