"""SimulationScaffolds, with the results of scripts/simulationScaffoldsRandom.py (mode 'random') and scripts/simulationScaffoldsByLength.py
(mode 'inv_length') of the reference: how far the completeness and contamination estimated from the marker sets of a lineage chain (and
from its refined twin) are off on a draft genome that lost whole scaffolds and gained scaffolds of a second genome, over the grid of
completeness and contamination levels (workers :71-165), and the two result files (writers :167-233).

The reference scores every marker set on every draw with two markerGenesOnScaffolds calls and MarkerSet.genomeCheck in both modes,
markers x copies x scaffolds Python iterations each.  Here all draws of a genome are made on the host, in the reference's order, so that
a seeded caller gets its scaffolds, and go to ONE MarkerSetBuilder.scaffoldChecks call (kernels_simscaf.hip).  The
chains come from MarkerSetBuilder.buildBinMarkerSet or buildBinMarkerSetsLOO; the process pool and the queues are replaced by the single
device call.

Kept from the scripts: the contigLen loop that neither script uses repeats every setting once per contig length with fresh draws; the
by-length script removes one scaffold at completeness 1.0 and adds one contaminant scaffold at contamination 0.0 (its sampler takes a
sequence before it tests the target); the random script's true contamination is whatever 100.0 - retained gives.  One deviation: the
contaminant is random.sample(sorted(candidates), 1)[0] -- the reference samples from a set of strings, whose order depends on the hash
seed and which current Python refuses to sample from."""
from collections import defaultdict
import gzip
import random
import time

from numpy import abs, mean, std

from checkm_amd.markerSetBuilder import MarkerSetBuilder


class SimulationScaffolds(object):
    def __init__(self, markerSetBuilder=None, mode='random', contigLens=None, percentComps=None, percentConts=None):
        if mode not in ('random', 'inv_length'):
            raise ValueError("mode is 'random' or 'inv_length'")
        self.markerSetBuilder = markerSetBuilder if markerSetBuilder is not None else MarkerSetBuilder()
        self.mode = mode
        self.contigLens = [5000, 20000, 50000] if contigLens is None else list(contigLens)
        self.percentComps = [0.5, 0.7, 0.8, 0.9, 0.95, 1.0] if percentComps is None else list(percentComps)
        self.percentConts = [0.0, 0.05, 0.1, 0.15, 0.2] if percentConts is None else list(percentConts)
        self.last_timing = {}
        self.last_draws = []

    def _seq_lens(self, genomeId, seen):
        """(sequence id -> length in FASTA order, genome size) from the precomputeGenomeSeqLens cache, else read once per evaluate."""
        if genomeId not in seen:
            img = self.markerSetBuilder.img
            cached = img.cachedGenomeSeqLens
            seqLens = cached[genomeId] if cached and genomeId in cached else img._genomeSeqLens(genomeId)
            seen[genomeId] = (seqLens, sum(seqLens.values()))
        return seen[genomeId]

    def _draw(self, percentComp, percentCont, testSeqLens, genomeSize, candidates, seen):
        """One replicate: (kept scaffolds of the test genome, contaminant, its sampled scaffolds, trueComp, trueCont).  The generators
        are used in the reference's order: numpy for the test genome, random for the contaminant, numpy for its scaffolds."""
        builder = self.markerSetBuilder
        if self.mode == 'random':
            retained, trueComp = builder.sampleGenomeScaffoldsWithoutReplacement(percentComp, testSeqLens, genomeSize)
        else:
            removed, perRemoved = builder.sampleGenomeScaffoldsInvLength(1.0 - percentComp, testSeqLens, genomeSize)
            trueComp = 100.0 - perRemoved
            removed = set(removed)
            retained = [seqId for seqId in testSeqLens if seqId not in removed]
        contGenomeId = random.sample(candidates, 1)[0]
        contSeqLens, contGenomeSize = self._seq_lens(contGenomeId, seen)
        if self.mode == 'random':
            seqsToRetain, trueRetainedPer = builder.sampleGenomeScaffoldsWithoutReplacement(1 - percentCont, contSeqLens, contGenomeSize)
            sampled = set(contSeqLens.keys()).difference(seqsToRetain)
            trueCont = 100.0 - trueRetainedPer
        else:
            sampled, trueCont = builder.sampleGenomeScaffoldsInvLength(percentCont, contSeqLens, contGenomeSize)
        return [str(s) for s in retained], contGenomeId, sorted(str(s) for s in sampled), trueComp, trueCont

    def evaluate(self, testGenomeId, binMarkerSets, refinedBinMarkerSet, genomeIdsToTest, numReplicates, taxonomy):
        """One tuple per (contig length, completeness, contamination) setting, in the reference's loop order: what its worker puts on
        the writer's queue (:165).  genomeIdsToTest holds the contaminant candidates (the test genome itself is left out), taxonomy is
        the list of the genome's metadata (or the joined string).  The scaffolds of the markers come from
        precomputeGenomeFamilyScaffolds, the sequence lengths from precomputeGenomeSeqLens where it has run."""
        t = dict(unmodified=0.0, draws=0.0, checks=0.0, tuples=0.0)
        self.last_timing = t
        builder = self.markerSetBuilder
        chain, refined = list(binMarkerSets.markerSetIter()), list(refinedBinMarkerSet.markerSetIter())
        t0 = time.perf_counter()
        genePositions = builder.img.geneDistTable([testGenomeId], binMarkerSets.getMarkerGenes(), spacingBetweenContigs=0)[testGenomeId]
        unmodifiedComp, unmodifiedCont = {}, {}
        for ms in chain:
            hits = {mg: genePositions[mg] for mg in ms.getMarkerGenes() if mg in genePositions}
            unmodifiedComp[ms.lineageStr], unmodifiedCont[ms.lineageStr] = builder._genome_check_host(ms, hits)[:2]
        t['unmodified'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        seen = {}
        testSeqLens, genomeSize = self._seq_lens(testGenomeId, seen)
        candidates = sorted(set(genomeIdsToTest) - set([testGenomeId]))
        settings, draws = [], []
        for contigLen in self.contigLens:
            for percentComp in self.percentComps:
                for percentCont in self.percentConts:
                    settings.append((contigLen, percentComp, percentCont))
                    draws.extend(self._draw(percentComp, percentCont, testSeqLens, genomeSize, candidates, seen) for _ in range(numReplicates))
        self.last_draws = draws
        t['draws'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        checks = builder.scaffoldChecks(chain + refined, testGenomeId, [d[:3] for d in draws])
        t['checks'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        checks = checks.tolist()
        if not isinstance(taxonomy, str):
            taxonomy = ';'.join(taxonomy)
        results = []
        for k, (contigLen, percentComp, percentCont) in enumerate(settings):
            deltas = [defaultdict(list) for _ in range(8)]      # comp, cont, comp set, cont set; the same four of the refined chain
            trueComps, trueConts, numDescendants = [], [], {}
            for r in range(k * numReplicates, (k + 1) * numReplicates):
                trueComp, trueCont = draws[r][3], draws[r][4]
                trueComps.append(trueComp)
                trueConts.append(trueCont)
                for s, ms in enumerate(chain + refined):
                    if s < len(chain):
                        numDescendants[ms.lineageStr] = ms.numGenomes
                    into = deltas[:4] if s < len(chain) else deltas[4:]
                    for d, value, true in zip(into, checks[r][s], (trueComp, trueCont, trueComp, trueCont)):
                        d[ms.lineageStr].append(value - true)
            results.append((testGenomeId, contigLen, percentComp, percentCont, taxonomy, numDescendants, unmodifiedComp, unmodifiedCont) + tuple(deltas) + (trueComps, trueConts))
        t['tuples'] = time.perf_counter() - t0
        return results

    SUMMARY_HEADER = ('Genome Id\tContig len\t% comp\t% cont\tTaxonomy\tMarker set\t# descendants\tUnmodified comp\tUnmodified cont'
                      '\tIM comp\tIM comp std\tIM cont\tIM cont std\tMS comp\tMS comp std\tMS cont\tMS cont std'
                      '\tRIM comp\tRIM comp std\tRIM cont\tRIM cont std\tRMS comp\tRMS comp std\tRMS cont\tRMS cont std\n')
    REPLICATE_HEADER = ('Genome Id\tContig len\t% comp\t% cont\tTaxonomy\tMarker set\t# descendants\tUnmodified comp\tUnmodified cont'
                        '\tIM comp\tIM cont\tMS comp\tMS cont\tRIM comp\tRIM cont\tRMS comp\tRMS cont\tTrue Comp\tTrue Cont\n')

    def write(self, results, summaryFile, replicateFile):
        """The writer's two files (:167-231) for the tuples of evaluate (of one genome or of several, concatenated): a summary line and
        a line of all replicates per setting and marker set of the main chain; replicateFile is gzipped.  Unlike simulation.py's files
        the summary has no true-comp pair and the replicate file carries the true values only at its end.  The lines follow the keys of
        unmodifiedComp: a lineage the refined chain lacks gets nan and empty columns."""
        with open(summaryFile, 'w') as summaryOut, gzip.open(replicateFile, 'wt') as fout:
            summaryOut.write(self.SUMMARY_HEADER)
            fout.write(self.REPLICATE_HEADER)
            for item in results:
                testGenomeId, contigLen, percentComp, percentCont, taxonomy, numDescendants, unmodifiedComp, unmodifiedCont = item[:8]
                deltas, trueComps, trueConts = item[8:16], item[16], item[17]
                for markerSetId in unmodifiedComp:
                    head = testGenomeId + '\t%d\t%.2f\t%.2f' % (contigLen, percentComp, percentCont) + '\t' + taxonomy + '\t' + markerSetId + '\t' + str(numDescendants[markerSetId]) \
                        + '\t%.3f\t%.3f' % (unmodifiedComp[markerSetId], unmodifiedCont[markerSetId])
                    columns = [d.get(markerSetId, []) for d in deltas]
                    summaryOut.write(head)
                    for column in columns:
                        summaryOut.write('\t%.3f\t%.3f' % (mean(abs(column)), std(abs(column))))
                    summaryOut.write('\n')
                    fout.write(head)
                    for column in columns + [trueComps, trueConts]:
                        fout.write('\t%s' % ','.join(map(str, column)))
                    fout.write('\n')
