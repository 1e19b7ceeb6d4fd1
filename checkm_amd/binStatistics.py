"""Bin statistics on the MI355X (checkm/binStatistics.py): the storage/bin_stats.*.tsv files lineage_wf writes twice (tree and analyze
step) and qa reads for every column of the extended table.

calculate() reads the bins with the rules of CheckM's readFasta on the library's host threads (ckm_nucseq_read), counts bases, code
points and the contig pieces between runs of >= 10 'N' on the device (ckm_nucstats_run), reads genes.gff / genes.faa of every bin on
host threads (ckm_bin_genes_read) and does the remaining arithmetic per bin here, with the reference's float operations in its order.
There is no CPU path for the file pass: without a device calculate() logs an error and exits, as MarkerGeneFinder.find does.
"""
import logging
import math
import os
import sys

import numpy as np

from checkm_amd import _lib
from checkm_amd.common import binIdFromFilename, makeSurePathExists

MIN_SEQ_LEN_GC_STD = 1000          # checkm/defaultValues.py: sequences longer than this enter the GC standard deviation
CONTIG_BREAK = 'NNNNNNNNNN'
PRODIGAL_GFF = 'genes.gff'
PRODIGAL_AA = 'genes.faa'

# (FASTA, genes.gff, genes.faa) as (path, size, mtime_ns) -> the bin's statistics: lineage_wf computes the same file twice (tree and
# analyze step, checkm/main.py:174-176 and :370-372)
_reuse = {}


def _file_key(path):
    try:
        st = os.stat(path)
    except OSError:
        return (path, None, None)
    return (os.path.abspath(path), st.st_size, st.st_mtime_ns)


def read_fasta(path):
    """{id: sequence} as CheckM's readFasta builds it (checkm/util/seqUtils.py:180-211), read by the library (ckm_nucseq_read)."""
    b = _lib.NucSeqs([path])
    try:
        return {i: b.seq(k).decode('utf-8') for k, i in enumerate(b.ids())}
    finally:
        b.close()


def calculateN50(seqLens):
    """Length of the sequence at which, longest first, the running total reaches half of the total (checkm/util/seqUtils.py:288-300)."""
    half = sum(seqLens) / 2.0
    seqLens.sort(reverse=True)
    total = 0
    for n in seqLens:
        total += n
        if total >= half:
            return n


def _base_count(seq):
    s = seq.upper()
    return s.count('A'), s.count('C'), s.count('G'), s.count('T') + s.count('U')


def _gc_summary(per_seq):
    """GC and GC std from [(a, c, g, t+u, length)] in dict order (BinStatistics.calculateGC)."""
    tot_gc = tot_at = 0
    kept = []
    fracs = []
    for a, c, g, t, n in per_seq:
        gc, at = g + c, a + t
        tot_gc += gc
        tot_at += at
        frac = float(gc) / (gc + at) if gc + at > 0 else 0.0
        fracs.append(frac)
        if n > MIN_SEQ_LEN_GC_STD:
            kept.append(frac)
    GC = float(tot_gc) / (tot_gc + tot_at) if tot_gc + tot_at > 0 else 0.0
    var = 0
    if len(kept) > 1:
        var = np.mean([(x - GC) ** 2 for x in kept])
    return GC, math.sqrt(var), fracs


def _length_summary(scaffold_lens, contig_lens):
    return (max(scaffold_lens), max(contig_lens), sum(scaffold_lens), calculateN50(list(scaffold_lens)), calculateN50(list(contig_lens)),
            np.mean(scaffold_lens), np.mean(contig_lens), len(contig_lens))


class BinStatistics(object):
    """Statistics of genome bins: GC, GC std, genome size, ambiguous bases, scaffolds and contigs, N50, mean lengths, coding density,
    translation table and gene count (checkm/binStatistics.py)."""

    def __init__(self, threads=1):
        self.logger = logging.getLogger('timestamp')
        self.totalThreads = threads
        self.last_timing = {}

    def calculate(self, binFiles, outDir, binStatsFile):
        """Write storage/<binStatsFile>: one line `binId\\t{...}` per bin, in binFiles order."""
        from checkm_amd import runtime
        import time
        self.logger.info("Calculating genome statistics for %d bins on the device:" % len(binFiles))
        try:
            ctx = runtime.get_ctx()
        except Exception as e:
            self.logger.error("No usable MI355X (gfx950) device for the bin statistics: %s" % e)
            sys.exit(1)
        t = dict(read=0.0, upload=0.0, kernel=0.0, gff=0.0, host=0.0, write=0.0, bytes=0, reused=0)
        stats = {}
        todo = []
        for binFile in binFiles:
            binId = binIdFromFilename(binFile)
            binDir = os.path.join(outDir, 'bins', binId)
            makeSurePathExists(binDir)
            key = (_file_key(binFile), _file_key(os.path.join(binDir, PRODIGAL_GFF)), _file_key(os.path.join(binDir, PRODIGAL_AA)))
            if key in _reuse:
                stats[binFile] = _reuse[key]
                t['reused'] += 1
            else:
                todo.append((binFile, binId, binDir, key))
        budget = int(os.environ.get("CKM_NUCSTATS_BATCH_MB", "1024")) << 20
        k = 0
        while k < len(todo):
            size, z = 0, k
            while z < len(todo) and (z == k or size + os.path.getsize(todo[z][0]) <= budget):
                size += os.path.getsize(todo[z][0])
                z += 1
            batch = todo[k:z]
            k = z
            t0 = time.perf_counter()
            seqs = _lib.NucSeqs([b[0] for b in batch])
            try:
                t1 = time.perf_counter()
                r = _lib.nucstats(ctx, seqs)
                t2 = time.perf_counter()
                genes = _lib.bin_genes(seqs, [os.path.join(b[2], PRODIGAL_GFF) for b in batch], [os.path.join(b[2], PRODIGAL_AA) for b in batch])
                t3 = time.perf_counter()
                for f, (binFile, binId, binDir, key) in enumerate(batch):
                    s = self._bin_stats(binId, r, int(seqs.file_first[f]), int(seqs.file_first[f + 1]), genes[f])
                    if s is not None:
                        stats[binFile] = s
                        _reuse[key] = s
                t4 = time.perf_counter()
            finally:
                seqs.close()
            t['read'] += t1 - t0
            t['upload'] += r['ms_upload'] / 1e3
            t['kernel'] += (r['ms_count'] + r['ms_fill']) / 1e3
            t['gff'] += t3 - t2
            t['host'] += (t2 - t1) - (r['ms_upload'] + r['ms_count'] + r['ms_fill']) / 1e3 + (t4 - t3)
            t['bytes'] += r['bytes']
        t0 = time.perf_counter()
        with open(os.path.join(outDir, 'storage', binStatsFile), 'w') as fout:
            for binFile in binFiles:
                if binFile in stats:
                    fout.write(binIdFromFilename(binFile) + '\t' + str(stats[binFile]) + '\n')
        t['write'] = time.perf_counter() - t0
        self.last_timing = t

    def _bin_stats(self, binId, r, a, z, genes):
        count, po, pl = r['count'], r['piece_off'], r['piece_len']
        scaffold_lens = [int(x) for x in count[a:z, 6]]
        contig_lens = [int(x) for x in pl[int(po[a]):int(po[z])]]
        if not contig_lens:
            # the reference's max([]) ends its worker process and the bin gets no line (checkm/binStatistics.py:232)
            self.logger.error("Bin %s has no contig base (every sequence is empty or 'N'): it gets no line in the bin statistics." % binId)
            return None
        per_seq = [(int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[6])) for x in count[a:z]]
        GC, stdGC, _ = _gc_summary(per_seq)
        maxS, maxC, size, n50S, n50C, meanS, meanC, nC = _length_summary(scaffold_lens, contig_lens)
        st = {}
        st['GC'] = GC
        st['GC std'] = stdGC
        st['Genome size'] = size
        st['# ambiguous bases'] = int(count[a:z, 4].sum() + count[a:z, 5].sum())
        st['# scaffolds'] = z - a
        st['# contigs'] = nC
        st['Longest scaffold'] = maxS
        st['Longest contig'] = maxC
        st['N50 (scaffolds)'] = n50S
        st['N50 (contigs)'] = n50C
        st['Mean scaffold length'] = float(meanS)
        st['Mean contig length'] = float(meanC)
        coding, table, ngenes = genes
        if coding == -1:
            st['Coding density'], st['Translation table'], st['# predicted genes'] = -1, -1, -1
        else:
            st['Coding density'] = float(coding) / size
            st['Translation table'] = table
            st['# predicted genes'] = ngenes
        return st

    def calculateGC(self, seqs, seqStats=None):
        """GC of all sequences of the dict and the standard deviation of the per-sequence GC of those longer than 1000."""
        per_seq = []
        for seqId, seq in seqs.items():
            per_seq.append(_base_count(seq) + (len(seq),))
        GC, stdGC, fracs = _gc_summary(per_seq)
        if seqStats:
            for seqId, frac in zip(seqs.keys(), fracs):
                seqStats[seqId]['GC'] = frac
        return GC, stdGC

    def calculateSeqStats(self, scaffolds, seqStats=None):
        """(longest scaffold, longest contig, total, scaffold N50, contig N50, mean scaffold, mean contig, contigs, ambiguous bases)."""
        scaffold_lens, contig_lens = [], []
        ambiguous = 0
        for scaffoldId, scaffold in scaffolds.items():
            scaffold_lens.append(len(scaffold))
            pieces = [n for n in (len(p.replace('N', '')) for p in scaffold.split(CONTIG_BREAK)) if n > 0]
            contig_lens += pieces
            if seqStats:
                seqStats[scaffoldId]['Length'] = len(scaffold)
                seqStats[scaffoldId]['Total contig length'] = sum(pieces)
                seqStats[scaffoldId]['# contigs'] = len(pieces)
            ambiguous += scaffold.count('N') + scaffold.count('n')
        return _length_summary(scaffold_lens, contig_lens) + (ambiguous,)

    def calculateCodingDensity(self, outDir, scaffolds, genomeSize):
        """(coding bases / genome size, translation table, genes of genes.faa) of the bin directory outDir, (-1, -1, -1) without a GFF."""
        from checkm_amd.prodigal import ProdigalGeneFeatureParser
        gffFile = os.path.join(outDir, PRODIGAL_GFF)
        if not os.path.exists(gffFile):
            return -1, -1, -1
        parser = ProdigalGeneFeatureParser(gffFile)
        aaGenes = read_fasta(os.path.join(outDir, PRODIGAL_AA))
        coding = 0
        for scaffoldId in scaffolds.keys():
            coding += parser.codingBases(scaffoldId)
        return float(coding) / genomeSize, parser.translationTable, len(aaGenes)

    def sequenceStats(self, outDir, binFile):
        """Per-sequence GC, length, contig length, contigs, ORFs and coding bases of one bin."""
        seqs = read_fasta(binFile)
        seqStats = {seqId: {} for seqId in seqs}
        self.calculateGC(seqs, seqStats)
        self.calculateSeqStats(seqs, seqStats)
        aaFile = os.path.join(outDir, 'bins', binIdFromFilename(binFile), PRODIGAL_AA)
        if not os.path.exists(aaFile):
            # the reference's else branch reads a name its loop never bound (checkm/binStatistics.py:284-288)
            raise UnboundLocalError("cannot access local variable 'gene' where it is not associated with a value")
        for geneId, gene in read_fasta(aaFile).items():
            seqId = geneId[0:geneId.rfind('_')]
            seqStats[seqId]['# ORFs'] = seqStats[seqId].get('# ORFs', 0) + 1
            seqStats[seqId]['Coding bases'] = seqStats[seqId].get('Coding bases', 0) + len(gene) * 3
        return seqStats
