"""The reference distributions of `checkm outliers` and `dist_plot` from genomes alone: distributions/gc_dist.txt, cd_dist.txt and
td_dist.txt, which the reference builds with five scripts outside its package (scripts/distributionDeltaGC.py,
distributionDeltaCodingDensity.py, distributionDeltaTetraDiff.py, calculateBounds.py, calculateBoundsTD.py).  The reference has no
class for this; ReferenceDistributions restates the scripts' intended semantics (DESIGN §18 lists every deviation).

Per genome the sequences are joined into one scaffold (GC: no separator, TD: 'NNNN', CD: ten 'N') and, for each window size, windows
are drawn at random starts until numWindows are accepted.  The file is read with the rules of CheckM's readFasta (ckm_nucseq_read); the
counts of every drawn window come from the device (ckm_refdist_run: prefix counts at block checkpoints, so a window costs two prefix
rows and fewer than two blocks of text whatever its size), the tetranucleotide distance is formed there in numpy's summation order, the
coding bases per window come from the merged intervals of the GFF on the host (ckm_refdist_coding).  Every quotient is one float64
division of integers.  There is no CPU path for the device pass.

The stream of one (genome, statistic, window size) is random.Random("%s:%s:%s:%d" % (seed, genomeId, stat, w)), so all sizes go to the
device together: draw what is still needed, evaluate, keep the accepted ones in draw order, repeat with the shortfall.

A genome with non-ASCII characters is not sent to the device: the Python statements below compute it (same result) and a DEBUG line
names it.
"""
import logging
import os
import random
import sys
import time

import numpy as np

from checkm_amd import _lib

SEP_LEN = {'gc': 0, 'td': 4, 'cd': 10}
DRAW_LIMIT = 100


def _genome_id(path):
    name = os.path.basename(path)
    return name[0:name.rfind('.')] if '.' in name else name


def _gc_at(s):
    return s.count('C') + s.count('G'), s.count('A') + s.count('T') + s.count('U')


class _HostScaffold(object):
    """The evaluation of a non-ASCII genome: the scripts' own slices."""

    def __init__(self, seqs, stat):
        self.stat = stat
        s = ('N' * SEP_LEN[stat]).join(seqs)
        self.text = s if stat == 'td' else s.upper()
        self.length = len(self.text)

    def __call__(self, starts, sizes):
        from checkm_amd.genomicSignatures import GenomicSignatures
        gs = GenomicSignatures(4, 1)
        totals = np.zeros(138, dtype=np.uint64)
        if self.stat == 'td':
            with np.errstate(invalid='ignore'):
                sig = gs.seqSignature(self.text)
                td = np.array([np.sum(np.abs(sig - gs.seqSignature(self.text[s:s + w]))) for s, w in zip(starts, sizes)], dtype=np.float64)
            return dict(counts=None, td=td, totals=totals, sig=sig)
        totals[0], totals[1] = _gc_at(self.text)
        counts = np.array([_gc_at(self.text[s:s + w]) for s, w in zip(starts, sizes)], dtype=np.uint32).reshape(len(starts), 2)
        return dict(counts=counts, td=None, totals=totals)


class ReferenceDistributions(object):
    """Per-genome window samples and the percentile tables made from them."""

    def __init__(self, threads=1):
        """threads is accepted for the signature of CheckM's classes and not used: the library sizes its own host threads."""
        self.logger = logging.getLogger('timestamp')
        self.last_timing = {}
        self.block = 0                                             # positions per prefix checkpoint (0: the library's default, 256)
        self.budget_bytes = 0

    def windowSizes(self):
        """The 41 sizes of the scripts, ascending."""
        sizes = []
        for a, z, step in ((500, 1000, 100), (1000, 2000, 200), (2000, 5000, 500), (5000, 10000, 1000), (10000, 50000, 5000), (50000, 100000, 10000),
                           (100000, 400000, 100000), (400000, 1000001, 200000)):
            sizes += list(range(a, z, step))
        return sizes

    def writeScaffold(self, genomeFile, outFile):
        """What distributionDeltaCodingDensity.py handed to prodigal: '>' + id + '\\n' + the ten-N scaffold, no trailing newline."""
        seqs = _lib.NucSeqs([genomeFile])
        try:
            text = ('N' * 10).join(seqs.seq(i).decode('utf-8') for i in range(seqs.nseq)).upper()
        finally:
            seqs.close()
        with open(outFile, 'w') as f:
            f.write('>' + _genome_id(genomeFile) + '\n' + text)

    # ---- sampling ----------------------------------------------------------------------------------------------------------------------

    def _check(self, numWindows, windowSizes):
        if isinstance(numWindows, bool) or not isinstance(numWindows, (int, np.integer)) or numWindows < 1:
            raise ValueError('numWindows must be an integer of at least 1, not %r' % (numWindows,))
        sizes = self.windowSizes() if windowSizes is None else list(windowSizes)
        for w in sizes:
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1:
                raise ValueError('a window size must be an integer of at least 1, not %r' % (w,))
        return int(numWindows), [int(w) for w in sizes]

    def _sample(self, genomeFile, stat, numWindows, windowSizes, seed, gffFile=None):
        numWindows, sizes = self._check(numWindows, windowSizes)
        from checkm_amd import runtime
        genomeId = _genome_id(genomeFile)
        t0 = time.perf_counter()
        seqs = _lib.NucSeqs([genomeFile])
        dev = dict.fromkeys(('ms_scaffold', 'ms_upload', 'ms_blocks', 'ms_scan', 'ms_windows', 'ms_download'), 0.0)
        info = dict(windows=0, rounds=0, blocks=0, bytes=0, host=False)
        t_coding = 0.0
        try:
            t1 = time.perf_counter()
            if _lib.seq_lengths(seqs) != seqs.seq_bytes.tolist():
                self.logger.debug('Genome %s holds non-ASCII characters: its windows are computed on the host.' % genomeId)
                evaluate = _HostScaffold([seqs.seq(i).decode('utf-8') for i in range(seqs.nseq)], stat)
                L = evaluate.length
                info['host'] = True
            else:
                try:
                    ctx = runtime.get_ctx()
                except Exception as e:
                    self.logger.error("No usable MI355X (gfx950) device for the reference distributions: %s" % e)
                    sys.exit(1)
                L = int(seqs.seq_bytes.sum()) + SEP_LEN[stat] * max(0, seqs.nseq - 1)

                def evaluate(starts, sizes_):
                    r = _lib.refdist(ctx, seqs, stat, SEP_LEN[stat], starts, sizes_, block=self.block, budget_bytes=self.budget_bytes)
                    for k in dev:
                        dev[k] += r[k]
                    info['blocks'], info['bytes'] = int(r['blocks']), int(r['bytes'])
                    return r
            used = []
            for w in sizes:
                if L - w <= 0:
                    break
                used.append(w)
            rng = {w: random.Random("%s:%s:%s:%d" % (seed, genomeId, stat, w)) for w in used}
            vals, draws, failed = {w: [] for w in used}, dict.fromkeys(used, 0), set()
            head = None
            while True:
                starts, wsz = [], []
                for w in used:
                    k = numWindows - len(vals[w])
                    if w in failed or k == 0:
                        continue
                    k = min(k, DRAW_LIMIT * numWindows - draws[w])
                    if k == 0:
                        failed.add(w)
                        continue
                    draws[w] += k
                    starts += [rng[w].randint(0, L - w) for _ in range(k)]
                    wsz += [w] * k
                if head is not None and not starts:
                    break
                r = evaluate(starts, wsz)
                info['windows'] += len(starts)
                info['rounds'] += 1
                if stat == 'td':
                    if head is None:
                        c = r['totals'][2:].astype(np.float64)
                        with np.errstate(invalid='ignore'):
                            head = r['sig'] if 'sig' in r else c / np.sum(c)
                    for w, v in zip(wsz, r['td'].tolist()):
                        vals[w].append(v)
                    continue
                gc, at = r['counts'][:, 0].tolist(), r['counts'][:, 1].tolist()
                if stat == 'gc':
                    if head is None:
                        head = float(int(r['totals'][0])) / (int(r['totals'][0]) + int(r['totals'][1]))
                    for w, g, a in zip(wsz, gc, at):
                        if g + a < 0.9 * w:
                            continue
                        vals[w].append(float(g) / (g + a) - head)
                else:
                    tc = time.perf_counter()
                    coding, total = _lib.refdist_coding(gffFile, genomeId, starts, wsz)
                    t_coding += time.perf_counter() - tc
                    if head is None:
                        head = float(total) / (int(r['totals'][0]) + int(r['totals'][1]))
                    for w, g, a, c in zip(wsz, gc, at, coding.tolist()):
                        if g + a != w:
                            continue
                        vals[w].append(float(c) / (g + a) - head)
            if failed:
                w = next(x for x in used if x in failed)           # the scripts take the sizes one after the other: the first in the order given
                raise ValueError('genome %s: fewer than %d acceptable %s windows of size %d in %d draws' % (genomeId, numWindows, stat, w, DRAW_LIMIT * numWindows))
        finally:
            seqs.close()
        t2 = time.perf_counter()
        on_dev = sum(dev.values()) / 1e3
        self.last_timing = dict(read=t1 - t0, scaffold=dev['ms_scaffold'] / 1e3, copy_in=dev['ms_upload'] / 1e3, blocks=dev['ms_blocks'] / 1e3, scan=dev['ms_scan'] / 1e3,
                                windows=dev['ms_windows'] / 1e3, copy_out=dev['ms_download'] / 1e3, coding=t_coding, python=(t2 - t1) - on_dev - t_coding,
                                drawn=info['windows'], rounds=info['rounds'], prefix_blocks=info['blocks'], bytes=info['bytes'], host=info['host'])
        return head, vals

    def deltaGC(self, genomeFile, numWindows=10000, windowSizes=None, seed=0):
        """(meanGC, {w: [GC of a window - meanGC]}) of one genome; ZeroDivisionError for a genome without a base."""
        return self._sample(genomeFile, 'gc', numWindows, windowSizes, seed)

    def deltaTD(self, genomeFile, numWindows=10000, windowSizes=None, seed=0):
        """(genome signature [136], {w: [Manhattan distance of a window's signature to it]}); nan for a window without a tetranucleotide."""
        return self._sample(genomeFile, 'td', numWindows, windowSizes, seed)

    def deltaCD(self, genomeFile, gffFile, numWindows=10000, windowSizes=None, seed=0):
        """(meanCD, {w: [coding density of a window - meanCD]}); gffFile: genes called on writeScaffold()'s file, seqid = genome id."""
        return self._sample(genomeFile, 'cd', numWindows, windowSizes, seed, gffFile=gffFile)

    # ---- files -------------------------------------------------------------------------------------------------------------------------

    @staticmethod
    def _fileText(stat, head, dist):
        if stat == 'td':
            text = '# Tetra signature = ' + ','.join(str(float(v)) for v in head) + '\n'
        else:
            text = '# Mean %s = %s\n' % (stat.upper(), str(float(head)))
        for w, vals in dist.items():
            text += 'Windows Size = ' + str(w) + '\n' + ','.join(str(float(v)) for v in vals) + '\n'
        return text

    def run(self, genomeFiles, outDir, gffFiles=None, numWindows=10000, windowSizes=None, seed=0):
        """Writes <outDir>/deltaGC|deltaTD|deltaCD/<genomeId>.tsv for every genome; deltaCD only with gffFiles (one per genome file)."""
        if gffFiles is not None and len(gffFiles) != len(genomeFiles):
            raise ValueError('gffFiles must name one GFF per genome file')
        timing = {}
        for k, genomeFile in enumerate(genomeFiles):
            jobs = [('gc', 'deltaGC', None), ('td', 'deltaTD', None)] + ([('cd', 'deltaCD', gffFiles[k])] if gffFiles is not None else [])
            for stat, sub, gff in jobs:
                head, dist = self._sample(genomeFile, stat, numWindows, windowSizes, seed, gffFile=gff)
                os.makedirs(os.path.join(outDir, sub), exist_ok=True)
                with open(os.path.join(outDir, sub, _genome_id(genomeFile) + '.tsv'), 'w') as f:
                    f.write(self._fileText(stat, head, dist))
                for key, v in self.last_timing.items():
                    if not isinstance(v, bool):
                        timing[key] = timing.get(key, 0) + v
        self.last_timing = timing

    # ---- bounds (host, numpy: np.percentile is the definition) ------------------------------------------------------------------------

    @staticmethod
    def _genomeFiles(genomeDir):
        return [(f[0:f.rfind('.')], os.path.join(genomeDir, f)) for f in sorted(os.listdir(genomeDir)) if f.endswith('.tsv')]

    @staticmethod
    def _windowLines(path):
        out, w = [], None
        with open(path) as f:
            for line in f:
                if 'Windows Size' in line:
                    w = int(line.split('=')[1].strip())
                elif w is not None:
                    out.append((w, line))
                    w = None
        return out

    @staticmethod
    def _percentiles(pts):
        CIs = np.arange(0, 100 + 0.5, 0.5).tolist()
        return {ci: float(p) for ci, p in zip(CIs, np.percentile(np.array(pts), CIs))}

    def bounds(self, genomeDir, outputFile, stepSize=0.01, width=0.015, minGenomes=5):
        """calculateBounds.py: {mean: {windowSize: {percentile: value}}} over the deltaGC or deltaCD files of genomeDir, written as str(dict)."""
        files = self._genomeFiles(genomeDir)
        means = {}
        for genomeId, path in files:
            with open(path) as f:
                means[genomeId] = float(f.readline().split('=')[1])
        paths = dict(files)
        dist = {}
        for centre in np.arange(0.0, 1.0 + 0.5 * stepSize, stepSize):
            ids = [g for g, v in means.items() if v >= centre - width and v <= centre + width]
            if len(ids) < minGenomes:
                continue
            d = {}
            for g in ids:
                for w, line in self._windowLines(paths[g]):
                    d.setdefault(w, []).extend(float(x) for x in line.split(','))
            dist[float(centre)] = {w: self._percentiles(pts) for w, pts in d.items()}
        with open(outputFile, 'w') as f:
            f.write(str(dist))
        return dist

    def boundsTD(self, genomeDir, outputFile, seed=0, maxPoints=10000):
        """calculateBoundsTD.py: {windowSize: {percentile: value}} over the deltaTD files of genomeDir, written as str(dict).  A line with
        a nan is left out and its genome reported; a line of more than maxPoints values is thinned.  Returns (dist, badGenomes)."""
        windows, bad = {}, []
        for genomeId, path in self._genomeFiles(genomeDir):
            for w, line in self._windowLines(path):
                if 'nan' in line:
                    if genomeId not in bad:
                        bad.append(genomeId)
                    continue
                vals = [float(x) for x in line.split(',')]
                if len(vals) > maxPoints:
                    vals = random.Random("%s:%s:%d" % (seed, genomeId, w)).sample(vals, maxPoints)
                windows.setdefault(w, []).extend(vals)
        dist = {w: self._percentiles(pts) for w, pts in windows.items()}
        with open(outputFile, 'w') as f:
            f.write(str(dist))
        return dist, bad
