"""Decoration of the genome tree: scripts/genometreeworkflow/decorateTree.py of the reference, which numbers the internal nodes, names
each after the taxon its genomes share, keeps its bootstrap value and writes genome_tree.metadata.tsv with the node's statistics and
marker set -- what MarkerSetBuilder.readNodeMetadata, TreeParser.readNodeMetadata and the tree walks read.  The marker sets of ALL nodes
come from one MarkerSetBuilder.buildMarkerSets call on the resident table; the rest is host work on treeParser's tree.

Declared deviations: rows are written in UID order (the reference's order is whatever its worker queue gave); the members
of a marker set are written sorted, in the `set([...])` spelling of the data files; labels that the taxa tree does not hold are skipped
when the common ancestor is looked for, and a node with none of its labels there gets the taxonomy ''; without a Pfam model file the
pfam ids stay as they are; numbers are written with Python 3's str.
"""
import numpy as np

from .markerSetBuilder import MarkerSetBuilder
from .treeParser import Tree, write_newick


def internalNodes(tree):
    """The internal nodes in pre-order, the root first (dendropy's internal_nodes())."""
    out, stack = [], [tree.root]
    while stack:
        v = stack.pop()
        if v.children:
            out.append(v)
            stack.extend(reversed(v.children))
    return out


def mrca(tree, labels, depth=None):
    """The most recent common ancestor of the leaves of that name in the tree; names the tree does not hold are skipped; None when it
    holds none of them.  depth: {id(node): depth} of the tree, made when absent."""
    if depth is None:
        depth = depthOf(tree)
    cur = None
    for label in labels:
        v = tree.find_leaf(label)
        if v is None:
            continue
        if cur is None:
            cur = v
            continue
        a, b = cur, v
        while depth[id(a)] > depth[id(b)]:
            a = a.parent
        while depth[id(b)] > depth[id(a)]:
            b = b.parent
        while a is not b:
            a, b = a.parent, b.parent
        cur = a
    return cur


def depthOf(tree):
    depth, stack = {id(tree.root): 0}, [tree.root]
    while stack:
        v = stack.pop()
        for c in v.children:
            depth[id(c)] = depth[id(v)] + 1
            stack.append(c)
    return depth


def meanStd(metadata, genomeLabels, category):
    """decorateTree.py:48-56: numpy's mean and std over the values that are not 'NA'."""
    values = []
    for genomeId in genomeLabels:
        v = metadata[genomeId.replace('IMG_', '')][category]
        if v != 'NA':
            values.append(v)
    if not values:
        return np.float64('nan'), np.float64('nan')
    return np.mean(values), np.std(values)


def setLiteral(sets):
    """A list of sets as the data files spell it, members sorted: [set(['a', 'b']), set(['c'])]."""
    return '[' + ', '.join('set([' + ', '.join(repr(str(m)) for m in sorted(s)) + '])' for s in sets) + ']'


class DecorateTree(object):
    """img: the IMG reader of the trusted genomes; builder: the MarkerSetBuilder to ask (default: one over img); pfamHMMs: the Pfam model
    file whose ACC lines give the accessions of the pfam ids, or None to leave the ids as they are."""

    def __init__(self, img, builder=None, pfamHMMs=None):
        self.img = img
        self.markerSetBuilder = builder if builder is not None else MarkerSetBuilder(img)
        self.pfamHMMs = pfamHMMs

    def pfamIdToPfamAcc(self):
        """decorateTree.py:70-79."""
        out = {}
        with open(self.pfamHMMs) as fin:
            for line in fin:
                if 'ACC' in line:
                    acc = line.split()[1].strip()
                    out[acc.split('.')[0]] = acc
        return out

    @staticmethod
    def readDuplicateTaxa(derepFile):
        duplicateTaxa = {}
        with open(derepFile) as fin:
            for line in fin:
                lineSplit = line.rstrip().split()
                if len(lineSplit) > 1:
                    duplicateTaxa[lineSplit[0]] = lineSplit[1:]
        return duplicateTaxa

    def decorate(self, taxaTreeFile, derepFile, inputTreeFile, metadataOut, ubiquityThreshold=0.97, singleCopyThreshold=0.97):
        """Numbers the internal nodes of inputTreeFile from 1 in pre-order, labels node n `UID<n>|<taxonomy>|<bootstrap>` (taxonomy: the
        label, spaces removed, of the common ancestor in the taxa tree of the node's leaves and their duplicates, '' when it has none;
        bootstrap: the node's old label or ''), writes the table metadataOut in UID order and rewrites inputTreeFile with the new
        labels.  Returns the rows written, as dicts."""
        metadata = self.img.genomeMetadata()
        duplicateTaxa = self.readDuplicateTaxa(derepFile)
        pfamIdToPfamAcc = self.pfamIdToPfamAcc() if self.pfamHMMs is not None else None
        taxaTree, inputTree = Tree.from_path(taxaTreeFile), Tree.from_path(inputTreeFile)
        depth = depthOf(taxaTree)
        rows = []
        for uniqueId, node in enumerate(internalNodes(inputTree), 1):
            labels = []
            for leaf in node.leaves():
                labels.append(leaf.taxon)
                labels.extend(duplicateTaxa.get(leaf.taxon, []))
            ancestor = mrca(taxaTree, labels, depth)
            taxaStr = ancestor.label.replace(' ', '') if ancestor is not None and ancestor.label else ''
            bootstrap = node.label if node.label else ''
            rows.append({'uid': uniqueId, 'node': node, 'labels': labels, 'taxonomy': taxaStr, 'bootstrap': bootstrap,
                         'label': 'UID' + str(uniqueId) + '|' + taxaStr + '|' + bootstrap})
        genomeLists = [list(dict.fromkeys(label.replace('IMG_', '') for label in r['labels'])) for r in rows]
        markerSets = self.markerSetBuilder.buildMarkerSets(genomeLists, ubiquityThreshold, singleCopyThreshold) if rows else []
        with open(metadataOut, 'w') as fout:
            fout.write('UID\t# genomes\tTaxonomy\tBootstrap')
            fout.write('\tGC mean\tGC std')
            fout.write('\tGenome size mean\tGenome size std')
            fout.write('\tGene count mean\tGene count std')
            fout.write('\tMarker set')
            fout.write('\n')
            for r, ms in zip(rows, markerSets):
                fout.write('UID' + str(r['uid']) + '\t' + str(len(r['labels'])) + '\t' + r['taxonomy'] + '\t' + r['bootstrap'])
                m, s = meanStd(metadata, r['labels'], 'GC %')
                fout.write('\t' + str(m * 100) + '\t' + str(s * 100))
                m, s = meanStd(metadata, r['labels'], 'genome size')
                fout.write('\t' + str(m) + '\t' + str(s))
                m, s = meanStd(metadata, r['labels'], 'gene count')
                fout.write('\t' + str(m) + '\t' + str(s))
                munged = []
                for geneSet in ms.markerSet:
                    out = set()
                    for geneId in geneSet:
                        if pfamIdToPfamAcc is not None and 'pfam' in geneId:
                            pfamId = geneId.replace('pfam', 'PF')
                            if pfamId in pfamIdToPfamAcc:
                                out.add(pfamIdToPfamAcc[pfamId])
                        else:
                            out.add(geneId)
                    munged.append(out)
                r['markerSet'] = munged
                fout.write('\t' + setLiteral(munged))
                fout.write('\n')
                r['node'].label = r['label']
        with open(inputTreeFile, 'w') as fout:
            fout.write(write_newick(inputTree) + '\n')
        return rows
