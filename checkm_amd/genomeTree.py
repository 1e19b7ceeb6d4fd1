"""The genome tree: the step of the reference's scripts/genometreeworkflow that hands the concatenated marker alignment to the external
program FastTree (inferGenomeTree.py), resamples its columns for bootstrap supports (bootstrapTree.py, with CompareToBootstrap.pl) and
roots the result between Archaea and Bacteria (rerootTree.py).  `concatenate`, `bootstrapColumns` and `reroot` keep the reference's
content; the tree itself is neighbour joining on corrected distances, on the device (checkm_amd/csrc/gtree_dev.h, kernels_gtree.hip,
DESIGN §27): pair counts over all rows, p / Poisson / Kimura distances with the library's own logarithm, and the joins of every tree of
a call driven from one stream.  No external program is looked for or run.

Declared deviations: neighbour joining on corrected distances instead of FastTree's WAG + gamma likelihood search; supports
written '%.3f' as the names of the internal nodes; the midpoint rule of `reroot` (dendropy is not used); file order where the order of a
Python 2 dict decided the reference's output.
"""
import bisect
import os
import random
import sys
from collections import defaultdict

import numpy as np

from . import _lib, runtime
from .pplacer import PNode, nodes_of, parse_newick, plain_name, quote_name, write_newick

RANK_PREFIXES = ('k__', 'p__', 'c__', 'o__', 'f__', 'g__', 's__')


def appendTaxonomyRanks(taxonomy, ranks=7):
    """The rank prefix in front of every taxon (checkm/util/taxonomyUtils.py:41-47)."""
    return [RANK_PREFIXES[i] + taxonomy[i] for i in range(ranks)]


def readFasta(path):
    """id (up to the first white space) -> sequence, in file order; a later record of an id replaces the sequence and keeps the place
    (checkm/util/seqUtils.py:180-211 on a dict that keeps insertion order)."""
    seqs, cur = {}, None
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            if line[0] == '>':
                cur = line[1:].split(None, 1)[0]
                seqs[cur] = []
            else:
                seqs[cur].append(line[0:-1])
    return {k: ''.join(v) for k, v in seqs.items()}


def _newick(root):
    """write_newick for trees of any depth: its walk is recursive, and a neighbour-joining tree of thousands of leaves can be a comb."""
    depth, stack = 0, [(root, 1)]
    while stack:
        v, d = stack.pop()
        depth = max(depth, d)
        stack.extend((c, d + 1) for c in v.children)
    limit = sys.getrecursionlimit()
    if 3 * depth + 200 <= limit:
        return write_newick(root)
    sys.setrecursionlimit(3 * depth + 200)
    try:
        return write_newick(root)
    finally:
        sys.setrecursionlimit(limit)


def _refuse(err):
    """A CkmError of the library as the ValueError the public calls raise: the message names the limit."""
    if isinstance(err, _lib.CkmError) and err.code in (-1, -7):
        return ValueError('GenomeTree: %s' % err)
    return err


class GenomeTree(object):
    """runner: what executes a _lib.GtreeTables call -- the device (default) or, in the CPU tests, the host executor."""

    def __init__(self, budget_bytes=0, runner=None):
        self.budget_bytes = budget_bytes
        self._runner = runner

    # ---- host part: the reference's files ----------------------------------------------------------------------------------------------
    @staticmethod
    def _genesInGenomes(img, genomeIds):
        """genome -> family -> gene -> the lowest e-value of its rows in the Pfam and TIGRFAM tables (inferGenomeTree.py:47-72)."""
        genesInGenomes = {}
        for genomeId in genomeIds:
            markerIdToGeneIds = defaultdict(dict)
            for ext, famCol, evalueCol in ((img.pfamExtension, 8, 6), (img.tigrExtension, 6, 4)):
                with open(os.path.join(img.genomeDir, genomeId, genomeId + ext)) as f:
                    f.readline()
                    for line in f:
                        lineSplit = line.split('\t')
                        famId, geneId, evalue = lineSplit[famCol], lineSplit[0], float(lineSplit[evalueCol])
                        markerIdToGeneIds[famId][geneId] = min(evalue, markerIdToGeneIds[famId].get(geneId, 1000))
            genesInGenomes[genomeId] = markerIdToGeneIds
        return genesInGenomes

    @staticmethod
    def _filterParalogs(seqs, markerId, genesInGenomes):
        """One sequence per genome (inferGenomeTree.py:74-105), exactly as written: the inner loop walks the ids after position i but
        looks their genome and gene up at positions 0, 1, ... of the list."""
        seqIds = list(seqs.keys())
        genomeIdGeneId = [seqId.split('|') for seqId in seqIds]
        filteredSeqs = {}
        for i, seqIdI in enumerate(seqIds):
            genomeIdI, geneIdI = genomeIdGeneId[i]
            if genomeIdI in filteredSeqs:
                continue
            geneIdToEvalue = genesInGenomes[genomeIdI][markerId]
            topHitId, topHitEvalue = seqIdI, geneIdToEvalue[geneIdI]
            for j, seqIdJ in enumerate(seqIds[i + 1:]):
                genomeIdJ, geneIdJ = genomeIdGeneId[j]
                if genomeIdI == genomeIdJ and geneIdToEvalue[geneIdJ] < topHitEvalue:
                    topHitId, topHitEvalue = seqIdJ, geneIdToEvalue[geneIdJ]
            filteredSeqs[genomeIdI] = seqs[topHitId]
        return filteredSeqs

    def concatenate(self, geneTreeDir, alignmentDir, extension, outputAlignFile, outputTaxonomy, img):
        """InferGenomeTree.run up to the FastTree call (inferGenomeTree.py:119-179): the taxonomy file of the trusted genomes and the
        concatenated alignment of the genes that have a tree.  Returns the alignment as {id: sequence} in the order written.  Where the
        reference walks a Python 2 dict or set the order here is file order: the metadata file's for the taxonomy, first appearance over
        the sorted alignment files for the genomes."""
        geneIds = set(f[0:f.find('.')] for f in os.listdir(geneTreeDir) if f.endswith('.tre'))
        metadata = img.genomeMetadata()
        trusted = list(metadata.keys())
        with open(outputTaxonomy, 'w') as fout:
            for genomeId in trusted:
                taxonomy = [x.replace('unclassified', '') for x in appendTaxonomyRanks(metadata[genomeId]['taxonomy'])]
                fout.write('IMG_' + genomeId + '\t' + '; '.join(taxonomy) + '\n')
        genesInGenomes = self._genesInGenomes(img, trusted)
        alignments, genomeIds = {}, {}
        for f in sorted(os.listdir(alignmentDir)):
            geneId = f[0:f.find('.')]
            if f.endswith(extension) and geneId in geneIds:
                imgGeneId = geneId.replace('PF', 'pfam') if geneId.startswith('PF') else geneId
                seqs = self._filterParalogs(readFasta(os.path.join(alignmentDir, f)), imgGeneId, genesInGenomes)
                for g in seqs:
                    genomeIds.setdefault(g, None)
                alignments[geneId] = seqs
        concatenatedSeqs = {}
        for geneId in sorted(alignments.keys()):
            seqs = alignments[geneId]
            alignLen = len(next(iter(seqs.values())))
            for genomeId in genomeIds:
                concatenatedSeqs['IMG_' + genomeId] = concatenatedSeqs.get('IMG_' + genomeId, '') + (seqs[genomeId] if genomeId in seqs else '-' * alignLen)
        with open(outputAlignFile, 'w') as fout:
            for seqId, seq in concatenatedSeqs.items():
                fout.write('>' + seqId + '\n')
                fout.write(seq + '\n')
        return concatenatedSeqs

    @staticmethod
    def bootstrapColumns(alignmentLen, numBootstraps):
        """The drawn columns [numBootstraps, alignmentLen] (bootstrapTree.py:44): one random.randint per column per replicate, in the
        reference's order, from the `random` module's state -- a caller that seeds it gets the reference's columns."""
        return np.array([[random.randint(0, alignmentLen - 1) for _ in range(alignmentLen)] for _ in range(numBootstraps)], dtype=np.uint32).reshape(numBootstraps, alignmentLen)

    # ---- the tree as PNodes -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _tree_of(ids, merge_ij, merge_len):
        slot = []
        for name in ids:
            v = PNode()
            v.name = quote_name(name)
            slot.append(v)
        for (i, j), (li, lj) in zip(merge_ij.tolist(), merge_len.tolist()):
            u = PNode()
            for c, length in ((slot[i], li), (slot[j], lj)):
                c.parent, c.length = u, repr(float(length))
                u.children.append(c)
            slot[i] = u
        return slot[int(merge_ij[-1][0])]

    @staticmethod
    def _splits_of_merges(n, merge_ij):
        """The clade of every join as a bit row over the leaves, made canonical (the side without leaf 0), sorted."""
        full, width = (1 << n) - 1, (n + 7) // 8
        side = [1 << k for k in range(n)]
        rows = []
        for i, j in merge_ij.tolist():
            side[i] |= side[j]
            rows.append((full ^ side[i] if side[i] & 1 else side[i]).to_bytes(width, 'little'))
        return sorted(rows)

    @staticmethod
    def _clades(root, index):
        """node -> the bit row (an int) of the leaves below it; index: plain leaf name -> bit."""
        clade = {}
        for v in nodes_of(root):                                    # post-order: children first
            if v.children:
                m = 0
                for c in v.children:
                    m |= clade[c]
                clade[v] = m
            else:
                name = plain_name(v.name)
                if name not in index:
                    raise ValueError('GenomeTree: the tree has the leaf %s, the alignment does not' % name)
                clade[v] = 1 << index[name]
        return clade

    # ---- device part ------------------------------------------------------------------------------------------------------------------
    def _run(self, tables, **what):
        try:
            if self._runner is not None:
                return self._runner(tables, budget_bytes=self.budget_bytes, **what)
            return _lib.gtree_run(runtime.get_ctx(), tables, budget_bytes=self.budget_bytes, **what)
        except _lib.CkmError as e:
            raise _refuse(e)

    @staticmethod
    def _rows(seqs):
        items = list(seqs.items()) if hasattr(seqs, 'items') else list(seqs)
        if len(items) < 2:
            raise ValueError('GenomeTree: a tree needs at least two rows')
        ids = [k for k, _ in items]
        if len(set(ids)) != len(ids):
            raise ValueError('GenomeTree: an id appears twice')
        ncols = len(items[0][1])
        for k, s in items:
            if len(s) != ncols:
                raise ValueError('GenomeTree: row %s has %d columns, the first row %d' % (k, len(s), ncols))
        if len(items) > _lib.GTREE_MAX_ROWS or ncols > _lib.GTREE_MAX_COLS:
            raise ValueError('GenomeTree: more than %d rows or more than %d columns' % (_lib.GTREE_MAX_ROWS, _lib.GTREE_MAX_COLS))
        try:
            text = b''.join(s if isinstance(s, bytes) else s.encode('ascii') for _, s in items)
        except UnicodeEncodeError:
            raise ValueError('GenomeTree: the alignment holds a character outside ASCII')
        return ids, text, ncols

    def _tables(self, seqs, cols=None, base=True, model='kimura', maxDist=3.0):
        if model not in _lib.GTREE_MODELS:
            raise ValueError("GenomeTree: model is 'kimura', 'poisson' or 'p'")
        ids, text, ncols = self._rows(seqs)
        return ids, _lib.GtreeTables(text=text, nrows=len(ids), ncols=ncols, cols=cols, base=base, model=model, max_dist=maxDist)

    def pairCounts(self, seqs):
        """(ids, compared, differ): per pair of rows the columns where both hold a residue, and those of them where the residues differ."""
        ids, t = self._tables(seqs)
        r = self._run(t, counts=True, merges=False)
        return ids, r['compared'], r['differ']

    def distances(self, seqs, model='kimura', maxDist=3.0):
        """(ids, matrix [n, n] float64)."""
        ids, t = self._tables(seqs, model=model, maxDist=maxDist)
        return ids, self._run(t, dist=True, merges=False)['dist']

    def neighbourJoin(self, ids, matrix):
        """Newick text of the neighbour-joining tree of a symmetric matrix."""
        m = np.asarray(matrix, dtype=np.float64)
        ids = list(ids)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] != len(ids):
            raise ValueError('GenomeTree: one row and one column per id')
        if len(ids) > _lib.GTREE_MAX_ROWS:
            raise ValueError('GenomeTree: more than %d rows' % _lib.GTREE_MAX_ROWS)
        if not np.array_equal(m, m.T):
            raise ValueError('GenomeTree: the matrix is not symmetric')
        r = self._run(_lib.GtreeTables(matrices=m[None]))
        return _newick(self._tree_of(ids, r['merge_ij'][0], r['merge_len'][0]))

    def infer(self, seqs, model='kimura', maxDist=3.0):
        """Newick text of the tree of an alignment {id: sequence}."""
        ids, t = self._tables(seqs, model=model, maxDist=maxDist)
        r = self._run(t)
        return _newick(self._tree_of(ids, r['merge_ij'][0], r['merge_len'][0]))

    def replicateSplits(self, seqs, numBootstraps=100, model='kimura', maxDist=3.0, cols=None):
        """Per replicate the sorted canonical bit rows of its tree's clades (cols: the drawn columns, else bootstrapColumns)."""
        ids, text, ncols = self._rows(seqs)
        cols = self.bootstrapColumns(ncols, numBootstraps) if cols is None else np.asarray(cols, dtype=np.uint32).reshape(-1, ncols)
        if cols.shape[0] == 0:
            return ids, []
        ids, t = self._tables(seqs, cols=cols, base=False, model=model, maxDist=maxDist)
        r = self._run(t)
        return ids, [self._splits_of_merges(len(ids), r['merge_ij'][k]) for k in range(cols.shape[0])]

    @classmethod
    def supportTree(cls, treeText, ids, replicateSplits):
        """treeText with, as the name of every internal node but the root, the share of the replicates whose tree holds the node's split,
        '%.3f'.  A split is compared as a whole bit row (a binary search over the replicate's sorted rows): no hash."""
        root = parse_newick(treeText)
        n, width = len(ids), (len(ids) + 7) // 8
        index = {name: k for k, name in enumerate(ids)}
        clade = cls._clades(root, index)
        full = (1 << n) - 1
        if clade[root] != full:
            raise ValueError('GenomeTree: the tree does not hold every row of the alignment once')
        for v in nodes_of(root):
            if not v.children or v.parent is None:
                continue
            row = (full ^ clade[v] if clade[v] & 1 else clade[v]).to_bytes(width, 'little')
            held = 0
            for rows in replicateSplits:
                at = bisect.bisect_left(rows, row)
                held += 1 if at < len(rows) and rows[at] == row else 0
            v.name = '%.3f' % (held / float(len(replicateSplits)) if replicateSplits else 0.0)
        return _newick(root)

    def bootstrap(self, seqs, treeText, numBootstraps=100, model='kimura', maxDist=3.0, cols=None):
        ids, splits = self.replicateSplits(seqs, numBootstraps, model, maxDist, cols)
        return self.supportTree(treeText, ids, splits)

    # ---- rooting ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def reroot(tree, outgroupLabels):
        """RerootTree.reroot (rerootTree.py:59-84) on a Newick text (returns text) or a PNode root (returns the new root).  If the
        outgroup is not empty, not every leaf, and one side of an edge holds exactly its leaves, the root goes on that edge, half its
        length to either side.  Otherwise the root goes to the midpoint of the longest leaf-to-leaf path; among paths of equal length the
        one whose leaves come first in the tree as written wins (path lengths are summed from the leaves up).  The outgroup's side, or the
        side of the path's first leaf, is written first.  A root of two children is dissolved first.  The name of an internal node (a
        support) belongs to the edge above it and moves with that edge."""
        as_text = not isinstance(tree, PNode)
        root = parse_newick(tree) if as_text else tree
        nodes = nodes_of(root)
        leaves = [v for v in nodes if not v.children]
        # the unrooted tree: adjacency lists (neighbour, length, label of the edge), children in order, the parent last
        adj = {v: [] for v in nodes}
        flen = lambda v: float(v.length) if v.length is not None else 0.0
        for v in nodes:
            for c in v.children:
                adj[v].append([c, flen(c), c.name if c.children else ''])
            if v.parent is not None:
                adj[v].append([v.parent, flen(v), v.name if v.children else ''])
        if len(root.children) == 2:
            a, b = root.children
            total, label = flen(a) + flen(b), (a.name if a.children else '') or (b.name if b.children else '')
            for x, y in ((a, b), (b, a)):
                for e in adj[x]:
                    if e[0] is root:
                        e[0], e[1], e[2] = y, total, label
            del adj[root]
            start = a if a.children else b
        else:
            start = root
        if len(adj) < 2:
            raise ValueError('GenomeTree: a tree of fewer than two leaves')
        # rooted at `start` for the walks below: order (parents first), up[v] = (parent, length, label)
        up, order = {start: None}, [start]
        for v in order:
            for w, length, label in adj[v]:
                if w not in up:
                    up[w] = (v, length, label)
                    order.append(w)
        leaf_at = {v: k for k, v in enumerate(leaves)}
        outgroup = set(outgroupLabels)
        inside = [v for v in leaves if plain_name(v.name) in outgroup]
        edge = None                                                    # (lower node, upper node, length, label, length on the lower side)
        if inside and len(inside) != len(leaves):
            count = {v: 0 for v in order}
            for v in inside:
                count[v] = 1
            for v in reversed(order):
                if up[v] is not None:
                    count[up[v][0]] += count[v]
            below = {v: 0 for v in order}
            for v in leaves:
                below[v] = 1
            for v in reversed(order):
                if up[v] is not None:
                    below[up[v][0]] += below[v]
            for v in order:
                if up[v] is None:
                    continue
                if (count[v] == len(inside) and below[v] == len(inside)) or (count[v] == 0 and len(leaves) - below[v] == len(inside)):
                    edge = (v, up[v][0], up[v][1], up[v][2], 0.5 * up[v][1])
                    low_first = count[v] != 0                        # the outgroup's side is written first
                    break
        if edge is None:
            # midpoint: per node the two farthest leaves below it through different children
            far = {}
            best = None
            for v in reversed(order):
                if v in leaf_at and v is not start:
                    far[v] = (0.0, leaf_at[v])
                    continue
                arms = sorted(((far[w][0] + length, far[w][1], w) for w, length, _ in adj[v] if up.get(w) is not None and up[w][0] is v and w in far),
                              key=lambda t: (-t[0], t[1]))
                if v in leaf_at:                                      # (the walk began at a leaf: only when the tree is two leaves)
                    arms.append((0.0, leaf_at[v], None))
                    arms.sort(key=lambda t: (-t[0], t[1]))
                if not arms:
                    continue
                far[v] = (arms[0][0], arms[0][1])
                if len(arms) >= 2:
                    cand = (-(arms[0][0] + arms[1][0]), min(arms[0][1], arms[1][1]), max(arms[0][1], arms[1][1]))
                    if best is None or cand < best[0]:
                        best = (cand, v, arms[0], arms[1])
            _, top, arm_a, arm_b = best
            half = 0.5 * (arm_a[0] + arm_b[0])
            # walk up from the farther leaf (arm_a) towards `top`
            v, cum = leaves[arm_a[1]], 0.0
            while True:
                parent, length, label = up[v]
                if cum + length >= half or parent is top:
                    edge = (v, parent, length, label, min(max(half - cum, 0.0), length))
                    low_first = arm_a[1] < arm_b[1]                  # the side of the path's first leaf is written first
                    break
                cum += length
                v = parent
        low, high, length, label, low_len = edge
        new_root = PNode()

        stack = [(high, low, new_root, length - low_len, label), (low, high, new_root, low_len, label)]
        if not low_first:
            stack.reverse()
        while stack:
            v, came_from, parent_node, ln, lb = stack.pop()
            node = PNode()
            node.parent, node.length = parent_node, repr(float(ln))
            node.name = lb if v.children else v.name                  # a leaf keeps its name, an internal node takes its edge's label
            parent_node.children.append(node)
            for w, wl, wlabel in reversed([e for e in adj[v] if e[0] is not came_from]):
                stack.append((w, v, node, wl, wlabel))
        fresh = parse_newick(_newick(new_root))                   # numbered as written
        return _newick(fresh) if as_text else fresh

    # ---- seqmagick --deduplicate-sequences -----------------------------------------------------------------------------------------------
    @staticmethod
    def deduplicate(alignFile, derepAlignFile, derepSeqFile):
        """Rows of alignFile with identical text collapse onto the first id in file order: derepAlignFile keeps the first occurrences in
        file order, derepSeqFile gets one line `kept dup1 dup2 ...` per kept id that has duplicates (what MarkerSetBuilder.readDuplicateSeqs
        and DecorateTree read).  A host dict; no kernel.  Returns {kept id: [duplicates]} for the ids that have any."""
        seqs = readFasta(alignFile)
        first, dups = {}, {}
        with open(derepAlignFile, 'w') as fout:
            for seqId, seq in seqs.items():
                if seq not in first:
                    first[seq] = seqId
                    fout.write('>' + seqId + '\n')
                    fout.write(seq + '\n')
                else:
                    dups.setdefault(first[seq], []).append(seqId)
        with open(derepSeqFile, 'w') as fout:
            for kept, others in dups.items():
                fout.write(' '.join([kept] + others) + '\n')
        return dups

    # ---- the reference's entry --------------------------------------------------------------------------------------------------------
    def run(self, geneTreeDir, alignmentDir, extension, outputAlignFile, outputTree, outputTaxonomy, bSupportValues=False, img=None, numBootstraps=100, model='kimura',
            maxDist=3.0):
        """InferGenomeTree.run (inferGenomeTree.py:119-190): the taxonomy file, the concatenated alignment and the tree, with bootstrap
        supports when bSupportValues is set.  img: the IMG reader of the trusted genomes."""
        if img is None:
            raise ValueError('GenomeTree.run needs the IMG reader of the trusted genomes (img=)')
        seqs = self.concatenate(geneTreeDir, alignmentDir, extension, outputAlignFile, outputTaxonomy, img)
        text = self.infer(seqs, model, maxDist)
        if bSupportValues:
            text = self.bootstrap(seqs, text, numBootstraps, model, maxDist)
        with open(outputTree, 'w') as fout:
            fout.write(text + '\n')
        return text
