"""Exploring and modifying bins (checkm/binTools.py): `checkm outliers`, `checkm modify`, `checkm unique`.

identifyOutliers() is the device path.  The tetranucleotide profile is parsed once by the library's host threads
(ckm_tetra_profile_read; the reference parses it once per bin), the bins are read with the rules of CheckM's readFasta
(ckm_nucseq_read) and counted on the device (ckm_nucstats_run), every sequence's coding bases come from its bin's genes.gff
(ckm_seq_genes_read), and one device pass (ckm_outliers_run) gives per sequence GC, coding density and tetranucleotide distance, their
differences to the bin and the outlier flags -- float64, bit for bit what the reference computes (the evaluation orders are stated in
checkm_amd/csrc/outlier_dev.h and, readably, by gcDist / codingDensityDist / binTetraSig / tetraDiffDist below).  Python picks the
bound tables per bin as the reference does and writes the rows of the flagged sequences.  There is no CPU path for this pass: without a
device identifyOutliers() logs an error and exits.

Declared differences: unique() prints the ids shared by two bins sorted (the reference prints them in set order), and the ids of an error
message of modify() / removeOutliers() are sorted too.  When a bin fails (ZeroDivisionError for a sequence without A, C, G, T, U;
KeyError for an id the profile does not hold; exit 1 for a missing genes.gff -- the reference's own failures, in its order), the rows of
the bins in front of it in the same batch are not written.
"""
import gzip
import logging
import os
import sys
import time

import numpy as np

from checkm_amd import _lib
from checkm_amd.common import binIdFromFilename, checkFileExists, findNearest, readDistribution
from checkm_amd.defaultValues import DefaultValues


def _read_fasta(path):
    """{id: sequence} as CheckM's readFasta builds it, read by the library (ckm_nucseq_read)."""
    b = _lib.NucSeqs([path])
    try:
        return {i: b.seq(k).decode('utf-8') for k, i in enumerate(b.ids())}
    finally:
        b.close()


def _write_fasta(seqs, outputFile):
    """`>id`, the sequence on one line (checkm/util/seqUtils.py writeFasta); a '.gz' name is compressed."""
    fout = gzip.open(outputFile, 'wt') if outputFile.endswith('.gz') else open(outputFile, 'w')
    with fout:
        for seqId, seq in seqs.items():
            fout.write('>' + seqId + '\n')
            fout.write(seq + '\n')


def _base_count(seq):
    s = seq.upper()
    return s.count('A'), s.count('C'), s.count('G'), s.count('T') + s.count('U')


class _Tables(object):
    """The bound tables of a batch as ckm_outliers_run takes them: one table per distinct (distribution, outer key), rows in the
    distribution's dict order."""

    def __init__(self):
        self.index, self.off, self.key, self.lo, self.hi, self.rows = {}, [0], [], [], [], []

    def add(self, name, byLen, loKey, hiKey):
        """Table of byLen = {seqLen: {percentile: bound}}; returns its index."""
        if name not in self.index:
            self.index[name] = len(self.off) - 1
            keys = list(byLen.keys())
            self.key += [float(k) for k in keys]
            self.lo += [float(byLen[k][loKey]) if loKey is not None else 0.0 for k in keys]
            self.hi += [float(byLen[k][hiKey]) if hiKey is not None else 0.0 for k in keys]
            self.off.append(len(self.key))
            self.rows.append(keys)
        return self.index[name]


class BinTools(object):
    """Functions for exploring and modifying bins."""

    def __init__(self, threads=1):
        self.logger = logging.getLogger('timestamp')
        self.last_timing = {}

    def _removeSeqs(self, seqs, seqsToRemove):
        missing = set(seqsToRemove).difference(seqs.keys())
        if missing:
            self.logger.error('Missing sequence(s) specified for removal: ' + ', '.join(sorted(missing)) + '\n')
            sys.exit(1)
        for seqId in seqsToRemove:
            seqs.pop(seqId)

    def _addSeqs(self, seqs, refSeqs, seqsToAdd):
        missing = set(seqsToAdd).difference(refSeqs.keys())
        if missing:
            self.logger.error('Missing sequence(s) specified for addition: ' + ', '.join(sorted(missing)) + '\n')
            sys.exit(1)
        for seqId in seqsToAdd:
            seqs[seqId] = refSeqs[seqId]

    def modify(self, binFile, seqFile, seqsToAdd, seqsToRemove, outputFile):
        """Write binFile plus the sequences seqsToAdd of seqFile minus the sequences seqsToRemove."""
        binSeqs = _read_fasta(binFile)
        if seqsToAdd is not None:
            self._addSeqs(binSeqs, _read_fasta(seqFile), seqsToAdd)
        if seqsToRemove is not None:
            self._removeSeqs(binSeqs, seqsToRemove)
        _write_fasta(binSeqs, outputFile)

    def removeOutliers(self, binFile, outlierFile, outputFile):
        """Write binFile without the sequences an identifyOutliers() file lists for this bin."""
        binSeqs = _read_fasta(binFile)
        binId = binIdFromFilename(binFile)
        checkFileExists(outlierFile)
        seqsToRemove = []
        with open(outlierFile) as f:
            for n, line in enumerate(f):
                cols = line.split('\t')
                if n > 0 and cols[0] == binId:
                    seqsToRemove.append(cols[1])
        if seqsToRemove:
            self._removeSeqs(binSeqs, seqsToRemove)
        _write_fasta(binSeqs, outputFile)

    def unique(self, binFiles):
        """Report sequences found twice in a bin and sequences assigned to several bins."""
        binSeqs = {}
        for f in binFiles:
            binId = binIdFromFilename(f)
            seqIds = set()
            with (gzip.open(f, 'rt') if f.endswith('.gz') else open(f)) as fin:
                for line in fin:
                    if line[0] == '>':
                        seqId = line[1:].split(None, 1)[0]
                        if seqId in seqIds:
                            print('  [Warning] Sequence %s found multiple times in bin %s.' % (seqId, binId))
                        seqIds.add(seqId)
            binSeqs[binId] = seqIds
        shared = False
        binIds = list(binSeqs.keys())
        for i in range(len(binIds)):
            for j in range(i + 1, len(binIds)):
                both = binSeqs[binIds[i]] & binSeqs[binIds[j]]
                if both:
                    shared = True
                    print('  Sequences shared between %s and %s: ' % (binIds[i], binIds[j]))
                    for seqId in sorted(both):
                        print('    ' + seqId)
                    print('')
        if not shared:
            print('  No sequences assigned to multiple bins.')

    # ---- the helpers the plot classes call; also the readable statement of what the device pass computes ---------------------------------

    def gcDist(self, seqs):
        """(GC of the bin, per-sequence GC minus it, per-sequence GC): every quotient is integer sums divided once."""
        GCs = []
        gcTotal = basesTotal = 0
        for seq in seqs.values():
            a, c, g, t = _base_count(seq)
            GCs.append(float(g + c) / (a + c + g + t))
            gcTotal += g + c
            basesTotal += a + c + g + t
        meanGC = float(gcTotal) / basesTotal
        return meanGC, np.array(GCs) - meanGC, GCs

    def codingDensityDist(self, seqs, prodigalParser):
        """(coding density of the bin, per-sequence density minus it, per-sequence density)."""
        CDs = []
        codingTotal = basesTotal = 0
        for seqId, seq in seqs.items():
            coding = prodigalParser.codingBases(seqId)
            CDs.append(float(coding) / len(seq))
            codingTotal += coding
            basesTotal += len(seq)
        meanCD = float(codingTotal) / basesTotal
        return meanCD, np.array(CDs) - meanCD, CDs

    def binTetraSig(self, seqs, tetraSigs):
        """Length-weighted sum of the sequences' signatures, in dict order: each row times its weight, then added to the running sum."""
        binSize = sum(len(seq) for seq in seqs.values())
        binSig = None
        for seqId, seq in seqs.items():
            weighted = tetraSigs[seqId] * (float(len(seq)) / binSize)
            if binSig is None:
                binSig = weighted
            else:
                binSig += weighted
        return binSig

    def tetraDiffDist(self, seqs, genomicSig, tetraSigs, binSig):
        """(mean, per-sequence) Manhattan distance between a sequence's signature and the bin's."""
        deltaTDs = np.zeros(len(seqs))
        for i, seqId in enumerate(seqs.keys()):
            deltaTDs[i] = genomicSig.distance(tetraSigs[seqId], binSig)
        return np.mean(deltaTDs), deltaTDs

    # ---- the device path ---------------------------------------------------------------------------------------------------------------

    def identifyOutliers(self, outDir, binFiles, tetraProfileFile, distribution, reportType, outputFile):
        """Write outputFile: a header and one row per sequence that lies outside the `distribution` percent bounds of the reference
        distributions of GC, coding density or tetranucleotide distance (reportType 'any') or of all three ('all')."""
        from checkm_amd import runtime
        self.logger.info('Reading reference distributions.')
        gcBounds = readDistribution('gc_dist')
        cdBounds = readDistribution('cd_dist')
        tdBounds = readDistribution('td_dist')
        try:
            ctx = runtime.get_ctx()
        except Exception as e:
            self.logger.error("No usable MI355X (gfx950) device for the outlier pass: %s" % e)
            sys.exit(1)
        t = dict(read=0.0, profile=0.0, genes=0.0, gather=0.0, nucstats=0.0, upload=0.0, seq=0.0, binsig=0.0, td=0.0, flags=0.0, host=0.0, write=0.0,
                 bins=len(binFiles), sequences=0, flagged=0)
        gcOuter, cdOuter = np.array(list(gcBounds.keys())), np.array(list(cdBounds.keys()))
        tdBoundKey = findNearest(list(tdBounds[list(tdBounds.keys())[0]].keys()), distribution)
        profile = None
        fout = open(outputFile, 'w')
        try:
            fout.write('Bin Id\tSequence Id\tSequence length\tOutlying distributions')
            fout.write('\tSequence GC\tMean bin GC\tLower GC bound (%s%%)\tUpper GC bound (%s%%)' % (distribution, distribution))
            fout.write('\tSequence CD\tMean bin CD\tLower CD bound (%s%%)' % distribution)
            fout.write('\tSequence TD\tMean bin TD\tUpper TD bound (%s%%)\n' % distribution)
            budget = int(os.environ.get("CKM_NUCSTATS_BATCH_MB", "1024")) << 20
            k = 0
            while k < len(binFiles):
                size, z = 0, k
                while z < len(binFiles) and (z == k or size + os.path.getsize(binFiles[z]) <= budget):
                    size += os.path.getsize(binFiles[z])
                    z += 1
                batch = binFiles[k:z]
                self.logger.info('Finding outliers in bins %d to %d of %d.' % (k + 1, z, len(binFiles)))
                k = z
                if profile is None:
                    t0 = time.perf_counter()
                    profile = _lib.TetraProfile(tetraProfileFile)
                    t['profile'] = time.perf_counter() - t0
                self._batch(ctx, outDir, batch, profile, gcBounds, cdBounds, tdBounds, gcOuter, cdOuter, tdBoundKey, distribution, reportType, fout, t)
        finally:
            fout.close()
            if profile is not None:
                profile.close()
        self.last_timing = t

    def _batch(self, ctx, outDir, batch, profile, gcBounds, cdBounds, tdBounds, gcOuter, cdOuter, tdBoundKey, distribution, reportType, fout, t):
        binIds = [binIdFromFilename(f) for f in batch]
        t0 = time.perf_counter()
        seqs = _lib.NucSeqs(batch)
        try:
            t1 = time.perf_counter()
            r = _lib.nucstats(ctx, seqs)
            t2 = time.perf_counter()
            coding, noGff = _lib.seq_genes(seqs, [os.path.join(outDir, 'bins', b, DefaultValues.PRODIGAL_GFF) for b in binIds])
            t3 = time.perf_counter()
            sig, firstMissing = profile.gather(seqs)
            t4 = time.perf_counter()
            ids = seqs.ids()
            first = [int(x) for x in seqs.file_first]
            count = r['count']
            gcn = (count[:, 2] + count[:, 1]).astype(np.int64)
            bases = (count[:, 0] + count[:, 1] + count[:, 2] + count[:, 3]).astype(np.int64)
            lens = count[:, 6].astype(np.int64)
            # the reference's failures, bin by bin in its order: gcDist divides, binTetraSig looks the ids up, then the GFF is asked for
            for f in range(len(batch)):
                a, z = first[f], first[f + 1]
                if a == z or (bases[a:z] == 0).any():
                    raise ZeroDivisionError('float division by zero')
                if a <= firstMissing < z:
                    raise KeyError(ids[firstMissing])
                if noGff[f]:
                    self.logger.error('Missing gene feature file (%s). This plot if not compatible with the --genes option.\n' % DefaultValues.PRODIGAL_GFF)
                    sys.exit(1)
            # the keys into the GC and CD distributions of every bin (integer sums divided once: what the device computes as well)
            tabs = _Tables()
            gcTab, cdTab, picked = [], [], []
            for f in range(len(batch)):
                a, z = first[f], first[f + 1]
                meanGC = float(int(gcn[a:z].sum())) / int(bases[a:z].sum())
                meanCD = float(int(coding[a:z].sum())) / int(lens[a:z].sum())
                closestGC = findNearest(gcOuter, meanGC)
                d = gcBounds[closestGC][list(gcBounds[closestGC].keys())[0]]
                gcLoKey = findNearest(list(d.keys()), (100 - distribution) / 2.0)
                gcHiKey = findNearest(list(d.keys()), (100 + distribution) / 2.0)
                closestCD = findNearest(cdOuter, meanCD)
                d = cdBounds[closestCD][list(cdBounds[closestCD].keys())[0]]
                cdLoKey = findNearest(list(d.keys()), (100 - distribution) / 2.0)
                gcTab.append(tabs.add(('gc', closestGC), gcBounds[closestGC], gcLoKey, gcHiKey))
                cdTab.append(tabs.add(('cd', closestCD), cdBounds[closestCD], cdLoKey, None))
                picked.append((meanGC, meanCD))
            tdTab = tabs.add(('td',), tdBounds, None, tdBoundKey)
            t5 = time.perf_counter()
            o = _lib.outliers(ctx, seqs, count, sig, coding, tabs.off, tabs.key, tabs.lo, tabs.hi, gcTab, cdTab, tdTab)
            t6 = time.perf_counter()
        finally:
            seqs.close()
        flags = o['flags']
        want = (flags != 0) if reportType == 'any' else (flags == 7) if reportType == 'all' else np.zeros(len(flags), dtype=bool)
        rows = []
        for f, binId in enumerate(binIds):
            a, z = first[f], first[f + 1]
            meanGC, meanCD = float(o['mean_gc'][f]), float(o['mean_cd'][f])
            if (meanGC, meanCD) != picked[f]:
                raise RuntimeError('bin %s: the device means (%r, %r) differ from the integer quotients (%r, %r)' % ((binId, meanGC, meanCD) + picked[f]))
            hit = np.nonzero(want[a:z])[0]
            if not len(hit):
                continue
            meanTD = np.mean(o['td'][a:z])
            gcKeys, cdKeys, tdKeys = tabs.rows[gcTab[f]], tabs.rows[cdTab[f]], tabs.rows[tdTab]
            g0, c0, t0_ = tabs.off[gcTab[f]], tabs.off[cdTab[f]], tabs.off[tdTab]
            for s in (a + int(x) for x in hit):
                n = int(lens[s])
                kg = g0 + gcKeys.index(findNearest(gcKeys, n))
                kc = c0 + cdKeys.index(findNearest(cdKeys, n))
                kt = t0_ + tdKeys.index(findNearest(tdKeys, n))
                gcLo, gcHi, cdLo, tdHi = tabs.lo[kg], tabs.hi[kg], tabs.lo[kc], tabs.hi[kt]
                fl = int(flags[s])
                rows.append(binId + '\t' + ids[s] + '\t%d' % n + '\t' + ','.join(nm for bit, nm in ((1, 'GC'), (2, 'CD'), (4, 'TD')) if fl & bit))
                rows.append('\t%.1f\t%.1f\t%.1f\t%.1f' % (float(o['gc'][s]) * 100, meanGC * 100, (meanGC + gcLo) * 100, (meanGC + gcHi) * 100))
                rows.append('\t%.1f\t%.1f\t%.1f' % (float(o['cd'][s]) * 100, meanCD * 100, (meanCD + cdLo) * 100))
                rows.append('\t%.3f\t%.3f\t%.3f' % (float(o['td'][s]), meanTD, tdHi) + '\n')
        fout.write(''.join(rows))
        t7 = time.perf_counter()
        dev = (o['ms_upload'] + o['ms_seq'] + o['ms_binsig'] + o['ms_td'] + o['ms_flags']) / 1e3
        t['read'] += t1 - t0
        t['nucstats'] += t2 - t1
        t['genes'] += t3 - t2
        t['gather'] += t4 - t3
        t['upload'] += o['ms_upload'] / 1e3
        t['seq'] += o['ms_seq'] / 1e3
        t['binsig'] += o['ms_binsig'] / 1e3
        t['td'] += o['ms_td'] / 1e3
        t['flags'] += o['ms_flags'] / 1e3
        t['host'] += (t5 - t4) + (t6 - t5) - dev
        t['write'] += t7 - t6
        t['sequences'] += len(flags)
        t['flagged'] += int(want.sum())
