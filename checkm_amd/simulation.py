"""Simulation, with the results of scripts/simulation.py of the reference: how far the completeness and contamination estimated from the
marker sets of a lineage chain (and from its refined twin) are off on draws of fixed-length contigs of a test genome, over the grid of
contig lengths, completeness and contamination levels (worker :97-145), and the two result files (writer :147-216).

The reference scores every marker set on every draw with containedMarkerGenes and MarkerSet.genomeCheck, markers x copies x contigs
Python iterations each.  Here all draws of a genome are made on the host, in the reference's order, so that a seeded caller gets its
contigs, and go to ONE MarkerSetBuilder.genomeChecks call (kernels_sim.hip).  The marker sets are the caller's: this
package's BinMarkerSets and MarkerSet, for instance from MarkerSetBuilder.buildBinMarkerSet.  The process pool and the queues are
replaced by the single device call."""
from collections import defaultdict
import gzip
import time

from numpy import abs, mean, std

from checkm_amd.markerSetBuilder import MarkerSetBuilder


class Simulation(object):
    def __init__(self, markerSetBuilder=None, contigLens=None, percentComps=None, percentConts=None):
        self.markerSetBuilder = markerSetBuilder if markerSetBuilder is not None else MarkerSetBuilder()
        self.contigLens = [1000, 2000, 5000, 10000, 20000, 50000] if contigLens is None else list(contigLens)
        self.percentComps = [0.5, 0.7, 0.8, 0.9, 0.95, 1.0] if percentComps is None else list(percentComps)
        self.percentConts = [0.0, 0.05, 0.1, 0.15, 0.2] if percentConts is None else list(percentConts)
        self.last_timing = {}

    def evaluate(self, testGenomeId, binMarkerSets, refinedBinMarkerSet, genePositions, genomeSize, numReplicates, taxonomy):
        """One tuple per (contig length, completeness, contamination) setting, in the reference's loop order: what its worker puts on
        the writer's queue (:145).  genePositions is geneDistTable[testGenomeId] for the markers of binMarkerSets, taxonomy the list of
        the genome's metadata (or the joined string)."""
        t = dict(unmodified=0.0, draws=0.0, checks=0.0, tuples=0.0)
        self.last_timing = t
        builder = self.markerSetBuilder
        chain, refined = list(binMarkerSets.markerSetIter()), list(refinedBinMarkerSet.markerSetIter())
        t0 = time.perf_counter()
        unmodifiedComp, unmodifiedCont = {}, {}
        for ms in chain:
            hits = {mg: genePositions[mg] for mg in ms.getMarkerGenes() if mg in genePositions}
            unmodifiedComp[ms.lineageStr], unmodifiedCont[ms.lineageStr] = builder._genome_check_host(ms, hits)[:2]
        t['unmodified'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        settings, draws = [], []
        for contigLen in self.contigLens:
            for percentComp in self.percentComps:
                for percentCont in self.percentConts:
                    settings.append((contigLen, percentComp, percentCont))
                    draws.extend(builder.sampleGenome(genomeSize, percentComp, percentCont, contigLen) for _ in range(numReplicates))
        t['draws'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        checks = builder.genomeChecks(chain + refined, genePositions, [d[2] for d in draws], [s[0] for s in settings for _ in range(numReplicates)])
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
                trueComp, trueCont = draws[r][0], draws[r][1]
                trueComps.append(trueComp)
                trueConts.append(trueCont)
                for s, ms in enumerate(chain + refined):
                    if s < len(chain):
                        numDescendants[ms.lineageStr] = ms.numGenomes
                    into = deltas[:4] if s < len(chain) else deltas[4:]
                    for d, value, true in zip(into, checks[r][s], (trueComp, trueCont, trueComp, trueCont)):
                        d[ms.lineageStr].append(value - true)
            results.append((testGenomeId, contigLen, percentComp, percentCont, taxonomy, numDescendants, unmodifiedComp, unmodifiedCont, trueComps, trueConts)
                           + tuple(deltas) + (trueComps, trueConts))
        t['tuples'] = time.perf_counter() - t0
        return results

    SUMMARY_HEADER = ('Genome Id\tContig len\t% comp\t% cont\tTaxonomy\tMarker set\t# descendants\tUnmodified comp\tUnmodified cont\tTrue comp\tTrue cont'
                      '\tIM comp\tIM comp std\tIM cont\tIM cont std\tMS comp\tMS comp std\tMS cont\tMS cont std'
                      '\tRIM comp\tRIM comp std\tRIM cont\tRIM cont std\tRMS comp\tRMS comp std\tRMS cont\tRMS cont std\n')
    REPLICATE_HEADER = ('Genome Id\tContig len\t% comp\t% cont\tTaxonomy\tMarker set\t# descendants\tUnmodified comp\tUnmodified cont\tTrue comp\tTrue cont'
                        '\tIM comp\tIM cont\tMS comp\tMS cont\tRIM comp\tRIM cont\tRMS comp\tRMS cont\tTrue Comp\tTrue Cont\n')

    def write(self, results, summaryFile, replicateFile):
        """The writer's two files (:147-216) for the tuples of evaluate (of one genome or of several, concatenated): a summary line and
        a line of all replicates per setting and marker set of the main chain; replicateFile is gzipped.  As in the reference the
        summary's "True comp / True cont" columns hold mean(trueComps) and std(trueConts), and the lines follow the keys of
        unmodifiedComp: a lineage the refined chain lacks gets nan and empty columns."""
        with open(summaryFile, 'w') as summaryOut, gzip.open(replicateFile, 'wt') as fout:
            summaryOut.write(self.SUMMARY_HEADER)
            fout.write(self.REPLICATE_HEADER)
            for item in results:
                testGenomeId, contigLen, percentComp, percentCont, taxonomy, numDescendants, unmodifiedComp, unmodifiedCont, trueComps, trueConts = item[:10]
                deltas = item[10:18]
                for markerSetId in unmodifiedComp:
                    head = testGenomeId + '\t%d\t%.2f\t%.2f' % (contigLen, percentComp, percentCont) + '\t' + taxonomy + '\t' + markerSetId + '\t' + str(numDescendants[markerSetId]) \
                        + '\t%.3f\t%.3f' % (unmodifiedComp[markerSetId], unmodifiedCont[markerSetId])
                    summaryOut.write(head + '\t%.3f\t%.3f' % (mean(trueComps), std(trueConts)))
                    for d in deltas:
                        summaryOut.write('\t%.3f\t%.3f' % (mean(abs(d[markerSetId])), std(abs(d[markerSetId]))))
                    summaryOut.write('\n')
                    fout.write(head)
                    for column in (trueComps, trueConts) + tuple(d[markerSetId] for d in deltas) + (trueComps, trueConts):
                        fout.write('\t%s' % ','.join(map(str, column)))
                    fout.write('\n')
