"""`checkm ssu_finder`: SSU rRNA genes on the contigs of an assembly (checkm/ssuFinder.py).  The reference pipes the assembly three
times through the external program nhmmer and post-processes its text report; here the three nucleotide models are scanned over both
strands of every contig on the device (checkm_amd/csrc/nhmm_dev.h states the scan, kernels_nhmm.hip runs it) and the
post-processing is kept byte for byte, quirks included: `bool('False')` is true, so strands never block concatenation; ids are
matched with the substring test `baseSeqId in curSeqId`; dicts keep insertion order; the gene is the slice `seq[start-1:end-1]` of the
forward strand; a gzipped bin file yields no ids (the reference compares a byte with '>').  No external program is looked for or run.

Declared deviations from nhmmer: the score is the Viterbi score of a unihit local alignment with the model's Viterbi Gumbel
(STATS LOCAL VITERBI), where nhmmer reports Forward-based i-Evalues after its domain definition, so E-values differ -- the coordinates
are what ssu_finder uses; no acceleration filter, every base meets every node; letters other than A C G T U score 0 at every node; a
contig file with a non-ASCII byte is refused; the constant -2.0 and the N / W scaling of the E-value are HMMER's as remembered, not
checked against the program; `ssu.<domain>.table.txt` is a tab format of our own and nhmmer's text report is not written; models hold
at most 2048 nodes.
"""
import logging
import math
import os
from collections import defaultdict

from . import _lib, runtime
from .common import binIdFromFilename
from .defaultValues import DefaultValues
from .hmmerModelParser import read_nuc_models

STRIDE = 16384                   # rows a tile owns; with overlap = MAXL part of the scan's definition, not a tuning knob
MIN_SCORE = -(1 << 20)           # nhmm_dev.h: no reporting threshold below this
MAX_SCORE = 1 << 28
LN2 = math.log(2.0)
TABLE_HEADER = '#target\tstrand\tfrom\tto\tscore_millibits\tE-value\n'


def _nhmm_run(tables, seqs, budget_bytes=0):
    """The device call (the tests put the host executor here)."""
    return _lib.nhmm_run(runtime.get_ctx(), tables, seqs, budget_bytes)


def evalue_of(score, W, mu, lam, N):
    """E-value of an integer milli-bit score: the window-length correction of a target of W positions, the model's Viterbi Gumbel,
    N / W windows in N positions."""
    bits = (score / 1000.0 * LN2 + 2.0 * math.log(2.0 / (W + 2.0)) - 2.0 - (W * math.log(W / (W + 1.0)) + math.log(1.0 / (W + 1.0)))) / LN2
    x = -lam * (bits - mu)
    p = 1.0 if x > 700.0 else -math.expm1(-math.exp(x))
    return p * N / W


def min_score_for(evalue, W, mu, lam, N):
    """The smallest integer score whose E-value is at most `evalue` (bisection: the E-value falls as the score rises), inside
    [MIN_SCORE, MAX_SCORE + 1]."""
    if evalue_of(MIN_SCORE, W, mu, lam, N) <= evalue:
        return MIN_SCORE
    if evalue_of(MAX_SCORE, W, mu, lam, N) > evalue:
        return MAX_SCORE + 1
    lo, hi = MIN_SCORE, MAX_SCORE                  # E(lo) > evalue >= E(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if evalue_of(mid, W, mu, lam, N) <= evalue:
            hi = mid
        else:
            lo = mid
    return hi


def filter_hits(hits, evalue):
    """The two filters, in order: E <= evalue (nhmmer's -E), then float('%.2g' % E) <= evalue (the reference's own test)."""
    return [h for h in hits if h['evalue'] <= evalue and float(h['printed']) <= evalue]


def readBinSeqIds(fastaFile):
    """The ids the reference's readFastaSeqIds gives: first word after '>'; none for a '.gz' file, whose lines it reads as bytes."""
    if fastaFile.endswith('.gz'):
        return []
    ids = []
    with open(fastaFile) as f:
        for line in f:
            if line[0] == '>':
                ids.append(line[1:].split(None, 1)[0])
    return ids


class SSU_Finder(object):
    def __init__(self, threads):
        self.logger = logging.getLogger('timestamp')
        self.totalThreads = threads
        ssu = os.path.join(DefaultValues.CHECKM_DATA_DIR, 'hmms_ssu')
        self.bacteriaModelFile = os.path.join(ssu, 'SSU_bacteria.hmm')
        self.archaeaModelFile = os.path.join(ssu, 'SSU_archaea.hmm')
        self.eukModelFile = os.path.join(ssu, 'SSU_euk.hmm')

    # ---- the scan ---------------------------------------------------------------------------------------------------------------------
    def _scanSeqs(self, modelFile, seqs, evalue, stride=STRIDE, budget_bytes=0, withInfo=False):
        models = read_nuc_models(modelFile)
        if len(models) != 1:
            raise ValueError('%s holds %d models, one is scanned' % (modelFile, len(models)))
        m = models[0]
        W = m.maxl
        N = 2 * int(sum(int(b) for b in seqs.seq_bytes))
        tables = _lib.NhmmTables([(m.emis, m.trans)], [min_score_for(evalue, W, m.mu, m.lam, N)], stride, W, 3)
        res = _nhmm_run(tables, seqs, budget_bytes)
        ids = seqs.ids()
        hits = []
        for k in range(len(res['hit_score'])):
            e = evalue_of(int(res['hit_score'][k]), W, m.mu, m.lam, N)
            hits.append(dict(seq=int(res['hit_seq'][k]), seqId=ids[int(res['hit_seq'][k])], rev=bool(res['hit_strand'][k]), start=int(res['hit_from'][k]),
                             end=int(res['hit_to'][k]), score=int(res['hit_score'][k]), evalue=e, printed='%.2g' % e))
        hits.sort(key=lambda h: (-h['score'], h['seq'], h['start']))
        hits = filter_hits(hits, evalue)
        return (hits, res) if withInfo else hits

    def scan(self, modelFile, contigFile, evalue):
        """The hits of one model on both strands of every contig of contigFile, best first: dicts with seqId, rev, start <= end on the
        forward strand (1-based, closed), score (milli-bits), evalue and printed ('%.2g' % evalue)."""
        seqs = _lib.NucSeqs([contigFile])
        try:
            return self._scanSeqs(modelFile, seqs, evalue)
        finally:
            seqs.close()

    def _hmmSearch(self, seqs, evalue, outputPrefix):
        found = {}
        for domain, label, modelFile in (('bacteria', 'bacterial 16S', self.bacteriaModelFile), ('archaea', 'archaeal 16S', self.archaeaModelFile),
                                         ('euk', 'eukaryotic 18S', self.eukModelFile)):
            self.logger.info('Identifying %s.' % label)
            found[domain] = self._scanSeqs(modelFile, seqs, evalue)
            with open(outputPrefix + '.' + domain + '.table.txt', 'w') as out:
                out.write(TABLE_HEADER)
                for h in found[domain]:
                    out.write('%s\t%s\t%d\t%d\t%d\t%s\n' % (h['seqId'], '-' if h['rev'] else '+', h['start'], h['end'], h['score'], h['printed']))
        return found

    # ---- the reference's post-processing ------------------------------------------------------------------------------------------------
    def _readHits(self, domainHits, domain, evalueThreshold):
        """What the reference parses out of a report: per sequence, in the order the sequences first appear, the hits in report order as
        [domain, E-value as printed, from, to, to - from, 'True' / 'False'] with from < to."""
        seqInfo = {}
        for h in domainHits:
            if float(h['printed']) <= evalueThreshold:
                info = [domain, h['printed'], str(h['start']), str(h['end']), str(h['end'] - h['start']), str(bool(h['rev']))]
                seqInfo[h['seqId']] = seqInfo.get(h['seqId'], []) + [info]
        return seqInfo

    def _addHit(self, hits, seqId, info, concatenateThreshold):
        """A hit of one model joins the hits of its sequence: fused with a near neighbour, else under the next free '-#n' name."""
        if seqId not in hits:
            hits[seqId] = info
            return
        base, n, fused, target = seqId, 1, False, seqId
        while True:
            newStart, newEnd = int(info[2]), int(info[3])
            oldStart, oldEnd = int(hits[seqId][2]), int(hits[seqId][3])
            # the reference compares bool(info[5]) with itself: strands never block
            span = None
            if abs(oldStart - newEnd) < concatenateThreshold:
                span = (newStart, oldEnd)
            elif abs(newStart - oldEnd) < concatenateThreshold:
                span = (oldStart, newEnd)
            if span is not None:
                del hits[seqId]
                info[2], info[3], info[4] = str(span[0]), str(span[1]), str(span[1] - span[0])
                hits[target] = info
                fused = True
            n += 1
            nextId = base + '-#' + str(n)
            if nextId in hits:
                seqId = nextId
                if not fused:
                    target = nextId
            else:
                if not fused:
                    hits[nextId] = info
                break

    def _addDomainHit(self, hits, baseSeqId, info):
        """A hit of one domain joins the best hits: dropped when it overlaps one at least as long, else it replaces those it overlaps."""
        newStart, newEnd, newLen = int(info[2]), int(info[3]), int(info[4])
        sameContig = [s for s in hits if baseSeqId in s]
        beaten = set()
        for s in sameContig:
            start, end, length = int(hits[s][2]), int(hits[s][3]), int(hits[s][4])
            if (newStart <= start and newEnd >= start) or (start <= newStart and end >= newStart):
                if newLen > length:
                    beaten.add(s)
                else:
                    return
        top = 0
        for s in sameContig:
            if s in beaten:
                del hits[s]
            elif '-#' in s:
                top = max(top, int(s.split('-#')[1]))
        hits['{}-#{}'.format(baseSeqId, top + 1)] = info

    @staticmethod
    def _baseId(seqId):
        return seqId[0:seqId.rfind('-#')] if '-#' in seqId else seqId

    def _postProcess(self, found, seqIdToBinId, seqOf, outputDir, evalueThreshold, concatenateThreshold):
        hitsPerDomain = {}
        for domain in ['archaea', 'bacteria', 'euk']:
            hits = {}
            for seqId, seqHits in self._readHits(found[domain], domain, evalueThreshold).items():
                for hit in seqHits:
                    self._addHit(hits, seqId, hit, concatenateThreshold)
            hitsPerDomain[domain] = hits
        bestHits = {}
        for hits in hitsPerDomain.values():
            for seqId, info in hits.items():
                self._addDomainHit(bestHits, self._baseId(seqId), info)
        relabelled, seen = {}, defaultdict(int)
        for seqId, info in bestHits.items():
            seqId = self._baseId(seqId)
            if seqId not in seen:
                relabelled[seqId] = info
            else:
                relabelled['{}-#{}'.format(seqId, seen[seqId])] = info
            seen[seqId] += 1
        bestHits = relabelled
        summaryFile = os.path.join(outputDir, 'ssu_summary.tsv')
        seqFile = os.path.join(outputDir, 'ssu.fna')
        hitsToBins = {}
        for name in bestHits:
            binId = seqIdToBinId.get(self._baseId(name), DefaultValues.UNBINNED)
            hitsToBins[binId] = hitsToBins.get(binId, []) + [[name] + bestHits[name]]
        with open(summaryFile, 'w') as summaryOut, open(seqFile, 'w') as seqOut:
            summaryOut.write('Bin Id\tSeq. Id\tHMM\ti-Evalue\tStart hit\tEnd hit\t16S/18S gene length\tRev. Complement\tSequence length\n')
            for binId in sorted(hitsToBins.keys()):
                for row in hitsToBins[binId]:
                    seq = seqOf(self._baseId(row[0]))
                    summaryOut.write(binId + '\t' + '\t'.join(row) + '\t' + str(len(seq)) + '\n')
                    seqOut.write('>' + binId + DefaultValues.SEQ_CONCAT_CHAR + row[0] + '\n')
                    seqOut.write(seq[int(row[3]) - 1:int(row[4]) - 1] + '\n')
        self.logger.info('Identified ' + str(len(bestHits)) + ' putative SSU genes.')
        self.logger.info('Summary of identified hits written to: ' + summaryFile)
        self.logger.info('SSU sequences written to: ' + seqFile)

    def run(self, contigFile, binFiles, outputDir, evalueThreshold, concatenateThreshold):
        if not os.path.exists(outputDir):
            os.makedirs(outputDir)
        self.logger.info('Determining bin assignment of sequences.')
        seqIdToBinId = {}
        for f in binFiles:
            binId = binIdFromFilename(f)
            for seqId in readBinSeqIds(f):
                seqIdToBinId[seqId] = binId
        self.logger.info('Identifying SSU rRNAs on sequences.')
        seqs = _lib.NucSeqs([contigFile])
        try:
            found = self._hmmSearch(seqs, evalueThreshold, os.path.join(outputDir, 'ssu'))
            index = dict((s, k) for k, s in enumerate(seqs.ids()))
            self._postProcess(found, seqIdToBinId, lambda seqId: seqs.seq(index[seqId]).decode('utf-8'), outputDir, evalueThreshold, concatenateThreshold)
        finally:
            seqs.close()
