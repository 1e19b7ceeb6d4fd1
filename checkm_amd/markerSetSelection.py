"""MarkerSetSelection, with the results of scripts/simInferBestMarkerSet.py and scripts/createSelectedMarkerSetMapping.py of the reference:
for every internal node of the genome tree the marker set of its ancestor chain that estimates completeness and contamination best on
sampled genomes of the node's smallest child lineage (that lineage left out when the sets are built), and from that table
selected_marker_sets.tsv, which MarkerSetParser.parseSelectedMarkerSetMap reads and lineage_wf scores bins with.

The reference draws 100 x 100 sampled genomes per node with Python's generators and scores every set of the chain on each in Python.
Here the draws of a node are made AND scored by one MarkerSetBuilder.sampledGenomeChecks call (kernels_select.hip):
draws='device'.  draws='host' makes them with random.uniform and sampleGenome in the script's order and scores them through genomeChecks,
so a caller that seeds both generators gets the reference's numbers.  The chains of all nodes come from one MarkerSetBuilder._chains call.

Deviations: the device stream is Philox4x32-10, not the Mersenne Twister, so device-mode numbers are not the reference's run for run; the
test genomes are random.sample of the SORTED child (the reference samples from a set, which current Python refuses); ties between sets
go to the first in chain order (the reference walks a Python 2 dict); run() gives every node its own seed (the reference's workers all
inherit one seeded generator, so its stream depends on their scheduling); the script's debugging exit on a completeness of 0.0 is
dropped."""
import random
import time
import zlib

import numpy as np
from numpy import abs, array, mean, std

from checkm_amd.markerSetBuilder import MarkerSetBuilder

NA = ('NA', -1, -1, -1, -1, -1)


def _fasta_bases(path):
    """Bases of a FASTA file: the characters of its sequence lines without trailing whitespace."""
    bases = 0
    with open(path) as f:
        for line in f:
            if line[0] != '>':
                bases += len(line.rstrip())
    return bases


def _internal_nodes(tree):
    """The internal nodes in preorder, the root first."""
    stack = [tree.root]
    while stack:
        node = stack.pop()
        if node.children:
            yield node
            stack.extend(reversed(node.children))


class MarkerSetSelection(object):
    HEADER = 'Internal node ID\tMarker set ID\tmean % delta comp\tstd % delta comp\tmean % delta cont\tstd % delta cont\n'

    def __init__(self, markerSetBuilder=None, simContigLen=10000):
        self.markerSetBuilder = markerSetBuilder if markerSetBuilder is not None else MarkerSetBuilder()
        self.simContigLen = simContigLen
        self.compRange, self.contRange = (0.5, 1.0), (0.0, 0.2)
        self.last_timing = {}
        self._in_run = False                         # run() adds its nodes' times up in one last_timing

    def _timing(self):
        return dict(chains=0.0, positions=0.0, pack=0.0, copy_in=0.0, kernel=0.0, copy_out=0.0, draws=0.0, checks=0.0, numpy=0.0, write=0.0, nodes=0, draws_made=0)

    def _genome_size(self, genomeId):
        """Bases of the genome's FASTA file (:91)."""
        return _fasta_bases(self.markerSetBuilder.img._path(genomeId, '.fna'))

    def _smallest_child(self, internalNode):
        """The genome ids below the child with the fewest (:59-75): its leaves and the genomes dereplicated into them."""
        duplicateSeqs = self.markerSetBuilder.duplicateSeqs
        leaves = []
        for child in internalNode.children:
            genomeIds = set()
            for leaf in child.leaves():
                genomeIds.add(leaf.taxon.replace('IMG_', ''))
                genomeIds.update(dup.replace('IMG_', '') for dup in duplicateSeqs.get(leaf.taxon, []))
            leaves.append(genomeIds)
        return sorted(leaves, key=len)[0]

    @staticmethod
    def node_seed(seed, internalNode):
        """The seed of a node: the caller's seed in the high half, a checksum of the node's UID in the low half."""
        return ((int(seed) & 0xffffffff) << 32) | zlib.crc32(internalNode.label.split('|')[0].encode())

    def selectMarkerSet(self, tree, internalNode, ubiquityThreshold, singleCopyThreshold, draws='device', seed=0, maxTestGenomes=100, repsPerGenome=100, chain=None):
        """(node label, bestUID, mean |delta comp|, its std, mean |delta cont|, its std) for the parent edge of internalNode (:56-129), or
        ('NA', -1, -1, -1, -1, -1) where the smallest child lineage has fewer than 5 genomes.  chain: the node's buildBinMarkerSet(...,
        bMarkerSet=False, genomeIdsToRemove=smallest child) where the caller has it already."""
        if draws not in ('device', 'host'):
            raise ValueError("draws is 'device' or 'host'")
        t = self.last_timing if self._in_run else self._timing()
        self.last_timing = t
        builder = self.markerSetBuilder
        smallest = self._smallest_child(internalNode)
        if len(smallest) < 5:
            return NA
        t0 = time.perf_counter()
        if chain is None:
            chain, _ = builder.buildBinMarkerSet(tree, internalNode, ubiquityThreshold, singleCopyThreshold, bMarkerSet=False, genomeIdsToRemove=smallest)
        t['chains'] += time.perf_counter() - t0
        testGenomeIds = random.sample(sorted(smallest), min(len(smallest), maxTestGenomes))
        sets = list(chain.markerSetIter())
        t0 = time.perf_counter()
        markerGenes = chain.getMarkerGenes()
        positions = [builder.img.geneDistTable([g], markerGenes, spacingBetweenContigs=0)[g] for g in testGenomeIds]
        sizes = [self._genome_size(g) for g in testGenomeIds]
        t['positions'] += time.perf_counter() - t0
        G, R, S = len(testGenomeIds), repsPerGenome, len(sets)
        if draws == 'device':
            true, out = builder.sampledGenomeChecks(sets, positions, sizes, R, self.simContigLen, self.compRange, self.contRange, seed)
            for k in ('pack', 'copy_in', 'kernel', 'copy_out'):
                t[k] += builder.last_select_timing[k]
        else:
            true, out = np.zeros((G, R, 2), dtype=np.float64), np.zeros((G, R, S, 4), dtype=np.float64)
            for g in range(G):
                t0 = time.perf_counter()
                starts = []
                for r in range(R):
                    testComp = random.uniform(*self.compRange)
                    testCont = random.uniform(*self.contRange)
                    true[g, r, 0], true[g, r, 1], contigs = builder.sampleGenome(sizes[g], testComp, testCont, self.simContigLen)
                    starts.append(contigs)
                t['draws'] += time.perf_counter() - t0
                t0 = time.perf_counter()
                if R:
                    out[g] = builder.genomeChecks(sets, positions[g], starts, [self.simContigLen] * R)
                t['checks'] += time.perf_counter() - t0
        t['nodes'] += 1
        t['draws_made'] += G * R
        t0 = time.perf_counter()
        deltaComp, deltaCont = {}, {}
        for s, ms in enumerate(sets):
            deltaComp.setdefault(ms.lineageStr, []).extend((out[:, :, s, 0] - true[:, :, 0]).reshape(-1).tolist())
            deltaCont.setdefault(ms.lineageStr, []).extend((out[:, :, s, 1] - true[:, :, 1]).reshape(-1).tolist())
        curBest, bestUID, dCompBest, dContBest, dCompStdBest, dContStdBest = 1000, None, 0, 0, 0, 0
        for lineageStr in deltaComp:                       # chain order
            dComp, dCont = mean(abs(array(deltaComp[lineageStr]))), mean(abs(array(deltaCont[lineageStr])))
            if (dComp + dCont) < curBest:
                dCompBest, dContBest = dComp, dCont
                dCompStdBest, dContStdBest = std(abs(array(deltaComp[lineageStr]))), std(abs(array(deltaCont[lineageStr])))
                bestUID = lineageStr.split('|')[0]
                curBest = dComp + dCont
        t['numpy'] += time.perf_counter() - t0
        return internalNode.label, bestUID, dCompBest, dCompStdBest, dContBest, dContStdBest

    def run(self, tree, ubiquityThreshold, singleCopyThreshold, outFile, draws='device', seed=0, maxTestGenomes=100, repsPerGenome=100):
        """The reference's table (:141-161) over every internal node that has a parent; returns the tuples, 'NA' nodes included.  Before
        every node both of Python's generators are seeded with the node's seed (node_seed), so a node's result does not depend on the
        nodes before it."""
        t = self._timing()
        self.last_timing, self._in_run = t, True
        builder = self.markerSetBuilder
        nodes = [n for n in _internal_nodes(tree) if n.parent is not None]
        eligible = [(n, self._smallest_child(n)) for n in nodes]
        eligible = [(n, smallest) for n, smallest in eligible if len(smallest) >= 5]
        t0 = time.perf_counter()
        chains = builder._chains(eligible, ubiquityThreshold, singleCopyThreshold, False) if eligible else []
        chain_of = {id(n): c[0] for (n, _), c in zip(eligible, chains)}
        t['chains'] += time.perf_counter() - t0
        results = []
        try:
            for node in nodes:
                nodeSeed = self.node_seed(seed, node)
                random.seed(nodeSeed)
                np.random.seed(nodeSeed & 0xffffffff)
                results.append(self.selectMarkerSet(tree, node, ubiquityThreshold, singleCopyThreshold, draws=draws, seed=nodeSeed, maxTestGenomes=maxTestGenomes,
                                                    repsPerGenome=repsPerGenome, chain=chain_of.get(id(node))))
        finally:
            self._in_run = False
        t0 = time.perf_counter()
        with open(outFile, 'w') as fout:
            fout.write(self.HEADER)
            for label, bestUID, dCompBest, dCompStdBest, dContBest, dContStdBest in results:
                if label != 'NA':
                    fout.write(label + '\t%s\t%.2f\t%.2f\t%.2f\t%.2f\n' % (bestUID, dCompBest, dCompStdBest, dContBest, dContStdBest))
        t['write'] += time.perf_counter() - t0
        return results

    @staticmethod
    def _inferred(node, inferredMarkerSet, domainUIDs):
        """The first ancestor-or-self with an inferred set other than 'NA'; a domain node answers for itself; else the root's UID."""
        while node is not None:
            uniqueId = node.label.split('|')[0]
            if inferredMarkerSet.get(uniqueId, 'NA') != 'NA':
                return inferredMarkerSet[uniqueId]
            if uniqueId in domainUIDs:
                return uniqueId
            node = node.parent
        return uniqueId

    def selectedMarkerSetMap(self, tree, inferredFile, outFile, domainUIDs=('UID2', 'UID203')):
        """selected_marker_sets.tsv (createSelectedMarkerSetMapping.py:62-87) from the table run() wrote: a line 'UID<tab>selected UID' per
        internal node.  Returns the mapping."""
        inferredMarkerSet = {}
        with open(inferredFile) as f:
            f.readline()
            for line in f:
                lineSplit = line.split('\t')
                inferredMarkerSet[lineSplit[0].split('|')[0].strip()] = lineSplit[1].split('|')[0].strip()
        selected = {}
        with open(outFile, 'w') as fout:
            for node in _internal_nodes(tree):
                uniqueId = node.label.split('|')[0]
                selected[uniqueId] = self._inferred(node, inferredMarkerSet, domainUIDs)
                fout.write(uniqueId + '\t' + selected[uniqueId] + '\n')
        return selected
