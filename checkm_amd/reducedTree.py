"""The reduced genome tree: scripts/genometreeworkflow/createSmallTree.py of the reference, which keeps one genome of every group of
nearly identical rows of the dereplicated concatenated alignment and prunes the genome tree to them, so that placement needs less
memory.  `nearlyIdentical` decides all pairs of rows in one device call (checkm_amd/csrc/nearid_dev.h, kernels_nearid.hip):
raw bytes, gaps included, eight columns per 64-bit operation, a bit per pair; the reference's greedy pass over the bit rows, the choice
of a member, the pruning and the files stay here.  No external program is looked for or run.

Declared deviations: clusters and their members follow the order of the alignment file where the order of a Python 2 dict
or set decided the reference's; `prune` states its own rule (dendropy's retain_taxa_with_labels is not used); no `taxit` reference
package and no FastTree log are made.
"""
import os
import random

import numpy as np

from . import _lib, runtime
from .genomeTree import readFasta
from .treeParser import Tree, write_newick


def plainNearlyIdentical(string1, string2, maxDiffPerc=0.08):
    """createSmallTree.py:65-75 as written: the zip stops at the shorter row; False at the difference that brings the count to
    int(maxDiffPerc * len(string1)) or beyond."""
    max_diff = int(maxDiffPerc * len(string1))
    n_diff = 0
    for c1, c2 in zip(string1, string2):
        if c1 != c2:
            n_diff += 1
            if n_diff >= max_diff:
                return False
    return True


def limitOf(row, maxDiffPerc=0.08):
    """The integer the device compares against: a pair is near iff diffs == 0 or diffs < int(maxDiffPerc * len(row)), which is
    diffs < max(that, 1).  The float expression is the reference's own."""
    return max(int(maxDiffPerc * len(row)), 1)


def prune(tree, keepLabels):
    """The tree (treeParser.Tree) cut down to the leaves named in keepLabels, in place; returns a Tree over the new root.  Leaves that are
    not kept are dropped; internal nodes left without leaves are dropped; a node left with one child is spliced out: the child keeps its
    own label and gets the sum of both branch lengths; a root left with one child is replaced by that child.  So every surviving
    internal node has at least two children, surviving nodes keep their labels, and the path length between two kept leaves is what it
    was wherever their common ancestor survives.  ValueError when no leaf is kept."""
    keep = set(keepLabels)
    order, stack = [], [tree.root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(reversed(v.children))
    wasLeaf = set(id(v) for v in order if not v.children)
    for v in reversed(order):                                         # children before their parents
        if id(v) in wasLeaf:
            continue
        kids = []
        for c in v.children:
            if id(c) in wasLeaf:
                if c.taxon in keep:
                    kids.append(c)
            elif len(c.children) == 1:
                g = c.children[0]
                if c.length is not None or g.length is not None:
                    g.length = (c.length or 0.0) + (g.length or 0.0)
                g.parent = v
                kids.append(g)
            elif c.children:
                kids.append(c)
        v.children = kids
    root = tree.root
    if id(root) not in wasLeaf and len(root.children) == 1:
        root = root.children[0]
        root.parent, root.length = None, None
    if (id(root) in wasLeaf and root.taxon not in keep) or (id(root) not in wasLeaf and not root.children):
        raise ValueError('ReducedTree: no leaf of the tree is kept')
    return Tree(root)


class ReducedTree(object):
    """runner: what executes a _lib.NearidTables call -- the device (default) or, in the CPU tests, the host executor."""

    def __init__(self, budget_bytes=0, runner=None):
        self.budget_bytes = budget_bytes
        self._runner = runner
        self.lastInfo = None                                       # counts and times of the last nearlyIdentical call

    def _run(self, tables):
        if self._runner is not None:
            return self._runner(tables, budget_bytes=self.budget_bytes)
        return _lib.nearid_run(runtime.get_ctx(), tables, budget_bytes=self.budget_bytes)

    @staticmethod
    def _plainClusters(ids, rows, maxDiffPerc):
        clusters, processed = [], [False] * len(ids)
        for i in range(len(ids)):
            if processed[i]:
                continue
            processed[i] = True
            members = [ids[i]]
            for j in range(i + 1, len(ids)):
                if not processed[j] and plainNearlyIdentical(rows[i], rows[j], maxDiffPerc):
                    members.append(ids[j])
                    processed[j] = True
            clusters.append(members)
        return clusters

    def nearlyIdentical(self, seqs, maxDiffPerc=0.08):
        """seqs: {id: row} in file order.  Returns the clusters of createSmallTree.py:91-119, each a list of ids in file order: for each
        row i in order that no earlier cluster took, the cluster is i and every later row j no cluster took yet that is nearly identical
        to i.  The relation is NOT transitive (a ~ b and b ~ c do not give a ~ c), so the clusters depend on the order of the rows: a
        chain a ~ b ~ c with a not near c gives [a, b], [c].  Rows of equal length are decided by one ckm_nearid_run call; unequal row
        lengths, an empty row, a character beyond one byte or a refusal by the library run the reference's plain loop with its truncating
        zip instead, counted in lastInfo['python_fallbacks']."""
        items = list(seqs.items()) if hasattr(seqs, 'items') else list(seqs)
        ids, rows = [k for k, _ in items], [s for _, s in items]
        info = {'python_fallbacks': 0, 'rows': len(ids), 'nbands': 0, 'npairs': 0, 'launches': 0, 'blocks': 0}
        self.lastInfo = info
        if not ids:
            return []
        near = None
        if len(rows[0]) > 0 and all(len(s) == len(rows[0]) for s in rows):
            try:
                tables = _lib.NearidTables([s if isinstance(s, bytes) else s.encode('latin-1') for s in rows], [limitOf(s, maxDiffPerc) for s in rows])
                o = self._run(tables)
                near = o['near']
                info.update({f: v for f, v in o.items() if f != 'near'})
            except UnicodeEncodeError:
                near = None
            except _lib.CkmError as e:
                if e.code not in (-1, -7):
                    raise
        if near is None:
            info['python_fallbacks'] = 1
            return self._plainClusters(ids, rows, maxDiffPerc)
        n = len(ids)
        clusters, processed = [], np.zeros(n, dtype=bool)
        for i in range(n):
            if processed[i]:
                continue
            processed[i] = True
            bits = np.unpackbits(near[i].astype('<u8').view(np.uint8), bitorder='little')[:n]
            js = np.nonzero(bits.astype(bool) & ~processed)[0]
            processed[js] = True
            clusters.append([ids[i]] + [ids[j] for j in js.tolist()])
        return clusters

    def nearlyIdenticalGenomes(self, seqs, outputDir):
        """createSmallTree.py:77-134: the clusters of <outputDir>/nearly_identical.tsv when the file exists (members in the file's order),
        else those of nearlyIdentical, written there one cluster per line, tab-separated."""
        path = os.path.join(outputDir, 'nearly_identical.tsv')
        numTaxa = 0
        if os.path.exists(path):
            identical = []
            with open(path) as fin:
                for line in fin:
                    members = []
                    for genomeId in line.split('\t'):
                        numTaxa += 1
                        if genomeId.strip() not in members:
                            members.append(genomeId.strip())
                    identical.append(members)
        else:
            identical = self.nearlyIdentical(seqs)
            numTaxa = len(identical)
            with open(path, 'w') as fout:
                for members in identical:
                    fout.write('\t'.join(members) + '\n')
        print('  Number of taxa: %d' % numTaxa)
        print('  Number of dereplicated taxa: %d' % len(identical))
        return identical

    def run(self, genomeTreeDir, outputDir):
        """createSmallTree.py:136-192 without its external programs: reads genome_tree.concatenated.derep.fasta and genome_tree.final.tre
        of genomeTreeDir; writes nearly_identical.tsv, genome_tree.fasta (one member per cluster, random.choice over the members in file
        order: seed `random` for a repeatable file), genome_tree.tre and genome_tree.small.no_internal_labels.tre into outputDir, which
        is then what PplacerRunner.place takes as alignment plus tree.  Returns the ids kept, in cluster order."""
        if not os.path.exists(outputDir):
            os.makedirs(outputDir)
        print('Filtering out highly similar taxa in order to reduce size of tree:')
        seqs = readFasta(os.path.join(genomeTreeDir, 'genome_tree.concatenated.derep.fasta'))
        clusters = self.nearlyIdenticalGenomes(seqs, outputDir)
        reducedSeqs = {}
        for members in clusters:
            rndGenome = random.choice(tuple(members))
            reducedSeqs[rndGenome] = seqs[rndGenome]
        with open(os.path.join(outputDir, 'genome_tree.fasta'), 'w') as fout:
            for seqId, seq in reducedSeqs.items():
                fout.write('>' + seqId + '\n')
                fout.write(seq + '\n')
        print('')
        print('Pruning tree:')
        tree = Tree.from_path(os.path.join(genomeTreeDir, 'genome_tree.final.tre'))
        for seqId in reducedSeqs:
            if tree.find_leaf(seqId) is None:
                print('Missing taxa: %s' % seqId)
        tree = prune(tree, reducedSeqs.keys())
        outputTree = os.path.join(outputDir, 'genome_tree.tre')
        with open(outputTree, 'w') as fout:
            fout.write(write_newick(tree) + '\n')
        for leaf in tree.root.leaves():
            if leaf.taxon not in reducedSeqs:
                print('missing in sequence file: %s' % leaf.taxon)
        with open(os.path.join(outputDir, 'genome_tree.small.no_internal_labels.tre'), 'w') as fout:
            fout.write(write_newick(tree, labels=False) + '\n')
        print('  Pruned tree written to: %s' % outputTree)
        return list(reducedSeqs)
