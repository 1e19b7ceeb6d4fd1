"""Gene trees and their two tests: the front of the reference's scripts/genometreeworkflow, which makes the directory of gene trees that
GenomeTree.run takes.  `makeTrees` (makeTrees.py) infers one tree per marker alignment, `paralogTest` (paralogTest.py) keeps a tree only
if the genomes with paralogous copies are conspecific below the copies' common ancestor, `consistencyTest` (consistencyTest.py) keeps a
tree only if its clades agree with domain, phylum and class; `run` chains the three in the reference's order.  The trees of a test are
scored in one device call (checkm_amd/csrc/genetree_dev.h, kernels_genetree.hip): the leaves of a tree are numbered in the
order they are written, a subtree is a leaf range and a count below a node a difference of two prefix sums.  Averages, formatting,
thresholds and file copies stay here.  No external program is looked for or run.

Declared deviations: the trees are GenomeTree's neighbour joining, not FastTree's WAG + gamma search, and makeTrees writes
no treeList.txt and no .log; rerooting is GenomeTree.reroot with its midpoint rule; sums and file columns follow first appearance among
the leaves where Python 2's dict order decided the reference's; str(float) is Python 3's; files are visited in sorted order.
"""
import math
import os
import shutil

import numpy as np

from . import _lib, runtime
from .genomeTree import GenomeTree, readFasta
from .pplacer import PNode, parse_newick, plain_name

NONE = _lib.GENETREE_NONE


def genomeIdOfLabel(taxaLabel):
    """The genome of a leaf label (consistencyTest.py:42-51, rerootTree.py:42-51)."""
    if taxaLabel.startswith('IMG_'):
        return taxaLabel[4:]
    if '|' in taxaLabel:
        return taxaLabel.split('|')[0]
    return taxaLabel


def genomeIdOfGene(taxaLabel):
    """The genome of a gene's label as paralogTest.py:103 reads it."""
    return taxaLabel.split('|')[0]


class PackedTree(object):
    """One tree as the device call takes it, with the names the reports need.  Arrays are per tree (positions and nodes count from 0)."""
    __slots__ = ('name', 'first', 'last', 'parent', 'length', 'internal', 'labels', 'genomes', 'leaf_genome', 'leaf_species', 'leaf_class', 'classes', 'totals', 'groups',
                 'pairs')


def packTree(name, tree, metadata, genomeId=genomeIdOfLabel):
    """tree: Newick text or a PNode root.  ValueError, naming the tree, for a leaf whose genome has no metadata, an edge without a length
    (the root's own aside) and a length that is no finite number."""
    root = tree if isinstance(tree, PNode) else parse_newick(tree)
    order, stack = [], [root]
    while stack:                                                      # pre-order as written
        v = stack.pop()
        order.append(v)
        stack.extend(reversed(v.children))
    at = {id(v): k for k, v in enumerate(order)}
    size = [0] * len(order)
    for k in range(len(order) - 1, -1, -1):
        v = order[k]
        size[k] = sum(size[at[id(c)]] for c in v.children) if v.children else 1
    p = PackedTree()
    p.name = name
    n = len(order)
    p.first, p.last, p.parent = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.full(n, NONE, dtype=np.uint32)
    p.length, p.internal = np.zeros(n), np.zeros(n, dtype=np.uint8)
    p.labels = []
    for k, v in enumerate(order):
        p.last[k] = p.first[k] + size[k]
        if v.parent is not None:
            if v.length is None:
                raise ValueError('GeneTrees: tree %s has an edge without a length' % name)
            try:
                p.length[k] = float(v.length)
            except ValueError:
                raise ValueError('GeneTrees: tree %s has the edge length %r' % (name, v.length))
        elif v.length is not None:
            p.length[k] = float(v.length)
        if not math.isfinite(p.length[k]):
            raise ValueError('GeneTrees: tree %s has an edge length that is not finite' % name)
        if v.children:
            p.internal[k] = 1
            pos = int(p.first[k])
            for c in v.children:
                j = at[id(c)]
                p.parent[j], p.first[j] = k, pos
                pos += size[j]
        else:
            p.labels.append(plain_name(v.name))
    nl = len(p.labels)
    p.genomes, p.leaf_genome, p.leaf_species = [], np.zeros(nl, dtype=np.uint32), np.full(nl, NONE, dtype=np.uint32)
    p.leaf_class, p.classes, p.totals = np.zeros((3, nl), dtype=np.uint32), [[], [], []], [[], [], []]
    genomeAt, speciesAt, classAt, members = {}, {}, [{}, {}, {}], []
    for k, label in enumerate(p.labels):
        g = genomeId(label)
        if g not in metadata:
            raise ValueError('GeneTrees: tree %s has the leaf %s, whose genome %s has no metadata' % (name, label, g))
        taxonomy = metadata[g]['taxonomy']
        if g not in genomeAt:
            genomeAt[g] = len(p.genomes)
            p.genomes.append(g)
            members.append([])
        p.leaf_genome[k] = genomeAt[g]
        members[genomeAt[g]].append(k)
        genus, sp = taxonomy[5], taxonomy[6].lower()
        if sp != '' and sp != 'unclassified' and genus != 'unclassified':
            p.leaf_species[k] = speciesAt.setdefault(genus + ' ' + sp, len(speciesAt))
        for r in range(3):
            c = classAt[r].get(taxonomy[r])
            if c is None:
                c = classAt[r][taxonomy[r]] = len(p.classes[r])
                p.classes[r].append(taxonomy[r])
                p.totals[r].append(0)
            p.leaf_class[r, k] = c
            p.totals[r][c] += 1
    p.groups = [gi for gi, m in enumerate(members) if len(m) > 1]
    p.pairs = [[(m[i], m[j]) for i in range(len(m)) for j in range(i + 1, len(m))] for m in (members[gi] for gi in p.groups)]
    return p


def withinLimits(p):
    return len(p.labels) <= _lib.GENETREE_MAX_LEAVES and len(p.first) <= _lib.GENETREE_MAX_NODES and max(len(c) for c in p.classes) <= _lib.GENETREE_MAX_CLASSES


def forestTables(packed):
    """The _lib.GenetreeTables of a list of PackedTree."""
    cat = lambda parts, dt: np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in parts]) if parts else np.zeros(0, dtype=dt)
    off = lambda counts: np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.uint32)
    return _lib.GenetreeTables(
        len(packed), node_off=off([len(p.first) for p in packed]), leaf_off=off([len(p.labels) for p in packed]),
        class_off=off([len(p.classes[r]) for p in packed for r in range(3)]), group_off=off([len(p.groups) for p in packed]),
        gpair_off=off([len(g) for p in packed for g in p.pairs]),
        first=cat([p.first for p in packed], np.uint32), last=cat([p.last for p in packed], np.uint32), parent=cat([p.parent for p in packed], np.uint32),
        length=cat([p.length for p in packed], np.float64), internal=cat([p.internal for p in packed], np.uint8),
        leaf_genome=cat([p.leaf_genome for p in packed], np.uint32), leaf_species=cat([p.leaf_species for p in packed], np.uint32),
        leaf_class=np.concatenate([p.leaf_class for p in packed], axis=1) if packed else np.zeros((3, 0), dtype=np.uint32),
        class_total=cat([t for p in packed for t in p.totals], np.uint32),
        pair_a=cat([[a for a, _ in g] for p in packed for g in p.pairs], np.uint32), pair_b=cat([[b for _, b in g] for p in packed for g in p.pairs], np.uint32))


def plainTreeTests(p):
    """The three outputs of one PackedTree by a plain Python loop: what runs in place of the library for a tree it refuses."""
    nl, nodes = len(p.labels), [k for k in range(len(p.first)) if p.internal[k]]
    first, last, parent, length = p.first.tolist(), p.last.tolist(), p.parent.tolist(), p.length.tolist()
    leafNode = [k for k in range(len(first)) if not p.internal[k]]
    consistency = []
    for r in range(3):
        cls = p.leaf_class[r].tolist()
        for c, T in enumerate(p.totals[r]):
            pre = [0]
            for x in cls:
                pre.append(pre[-1] + (1 if x == c else 0))
            best = 0.0
            for v in nodes:
                n, k = last[v] - first[v], pre[last[v]] - pre[first[v]]
                best = max(best, float(k) / float(T + (n - k)), float(T - k) / float(T + ((nl - n) - (T - k))))
            consistency.append(best)

    def rootDistance(v):
        d = length[v]
        v = parent[v]
        while v != NONE:
            d = d + length[v]
            v = parent[v]
        return d

    flags, groupNode, groupMixed = [], [], []
    species = p.leaf_species.tolist()
    for pairs in p.pairs:
        lo, hi = None, 0
        for a, b in pairs:
            va, vb = leafNode[a], leafNode[b]
            m = parent[va]
            while last[m] <= b:
                m = parent[m]
            if parent[m] == NONE:
                dist = rootDistance(va) + rootDistance(vb)
            else:
                dist, v = length[va], parent[va]
                while v != m:
                    dist, v = dist + length[v], parent[v]
                dist, v = dist + length[vb], parent[vb]
                while v != m:
                    dist, v = dist + length[v], parent[v]
            flags.append(1 if dist > 0 else 0)
            if dist > 0:
                lo, hi = a if lo is None else min(lo, a), max(hi, b)
        if lo is None:
            groupNode.append(NONE)
            groupMixed.append(0)
            continue
        node = max(v for v in nodes if first[v] <= lo and last[v] > hi)
        groupNode.append(node)
        groupMixed.append(1 if len(set(s for s in species[first[node]:last[node]] if s != NONE)) > 1 else 0)
    return (np.array(consistency, dtype=np.float64), np.array(flags, dtype=np.uint8), np.array(groupNode, dtype=np.uint32), np.array(groupMixed, dtype=np.uint8))


def _refuse(err, names):
    if isinstance(err, _lib.CkmError) and err.code in (-1, -7):
        return ValueError('GeneTrees: %s (trees of the call: %s)' % (err, ', '.join(names[:8]) + (', ...' if len(names) > 8 else '')))
    return err


class GeneTrees(object):
    """runner: what executes a _lib.GenetreeTables call -- the device (default) or, in the CPU tests, the emulator or the host executor.
    genomeTree: the GenomeTree whose `infer` makes the trees (default: one on the device)."""

    def __init__(self, budget_bytes=0, runner=None, genomeTree=None):
        self.budget_bytes = budget_bytes
        self._runner = runner
        self._genomeTree = genomeTree
        self.lastInfo = None                                       # counts and times of the last test's device call

    # ---- trees (makeTrees.py:38-65) ---------------------------------------------------------------------------------------------------
    def makeTrees(self, alignDir, outputDir, extension='.aln.masked.faa', model='kimura', maxDist=3.0):
        """Every alignment file with the extension is rewritten with '*' replaced by 'X' on its sequence lines, and its tree is written
        to <outputDir>/<prefix>.tre.  Returns the tree files written, in sorted order."""
        if not os.path.exists(outputDir):
            os.makedirs(outputDir)
        gt = self._genomeTree if self._genomeTree is not None else GenomeTree()
        written = []
        for f in sorted(os.listdir(alignDir)):
            if not f.endswith(extension):
                continue
            path = os.path.join(alignDir, f)
            with open(path) as fin:
                data = fin.readlines()
            with open(path, 'w') as fout:
                for line in data:
                    if line[0] != '>':
                        line = line.replace('*', 'X')
                    fout.write(line)
            prefix = f[0:f.rfind('.')]
            text = gt.infer(readFasta(path), model, maxDist)
            out = os.path.join(outputDir, prefix + '.tre')
            with open(out, 'w') as fout:
                fout.write(text + '\n')
            written.append(out)
        return written

    # ---- the device call --------------------------------------------------------------------------------------------------------------
    def _run(self, tables):
        if self._runner is not None:
            return self._runner(tables, budget_bytes=self.budget_bytes)
        return _lib.genetree_run(runtime.get_ctx(), tables, budget_bytes=self.budget_bytes)

    def treeTests(self, trees, metadata, genomeId=genomeIdOfLabel):
        """trees: [(name, Newick text or PNode root)] or {name: ...}; metadata: IMG.genomeMetadata().  All trees are scored in one device
        call.  Returns a dict of per-tree lists: 'packed' (the PackedTree: labels, genomes, classes, totals, groups, pairs), 'consistency'
        (float64, the classes of domain, phylum and class one after the other), 'pair_flag' (uint8, the pairs of the groups one after the
        other), 'group_node' (uint32, NONE: no flagged pair), 'group_mixed' (uint8); and 'info': the call's counts and times, with
        'python_trees', the trees beyond the library's limits that a plain Python loop scored instead."""
        items = list(trees.items()) if hasattr(trees, 'items') else list(trees)
        packed = [packTree(name, tree, metadata, genomeId) for name, tree in items]
        onDevice = [k for k, p in enumerate(packed) if withinLimits(p)]
        res = {f: [None] * len(packed) for f in ('consistency', 'pair_flag', 'group_node', 'group_mixed')}
        info = {'python_trees': len(packed) - len(onDevice), 'nrounds': 0, 'ntrees': 0, 'launches': 0}
        if onDevice:
            tables = forestTables([packed[k] for k in onDevice])
            try:
                o = self._run(tables)
            except _lib.CkmError as e:
                raise _refuse(e, [packed[k].name for k in onDevice])
            info.update({f: v for f, v in o.items() if f not in res})
            for i, k in enumerate(onDevice):
                c0, c1 = int(tables.class_off[3 * i]), int(tables.class_off[3 * i + 3])
                g0, g1 = int(tables.group_off[i]), int(tables.group_off[i + 1])
                p0, p1 = int(tables.gpair_off[g0]), int(tables.gpair_off[g1])
                res['consistency'][k], res['pair_flag'][k] = o['consistency'][c0:c1].copy(), o['pair_flag'][p0:p1].copy()
                res['group_node'][k], res['group_mixed'][k] = o['group_node'][g0:g1].copy(), o['group_mixed'][g0:g1].copy()
        for k, p in enumerate(packed):
            if res['consistency'][k] is None:
                res['consistency'][k], res['pair_flag'][k], res['group_node'][k], res['group_mixed'][k] = plainTreeTests(p)
        res['packed'], res['info'] = packed, info
        return res

    @staticmethod
    def _treeFiles(geneTreeDir, extension):
        return [f for f in sorted(os.listdir(geneTreeDir)) if f.endswith(extension)]

    # ---- paralogTest.py:67-161 --------------------------------------------------------------------------------------------------------
    def paralogTest(self, geneTreeDir, metadata, acceptPer=0.01, extension='.tre', outputDir='./data/gene_trees_conspecific/'):
        """One record per tree, in sorted file order: {'geneId', 'numTaxa', 'paralogs': sorted genomes with paralogous copies (same-genome
        leaves at a patristic distance > 0 in the rerooted tree), 'nonConspecific': sorted genomes among them with more than one counted
        species below the copies' common ancestor, 'retained'}.  outputDir is emptied and receives the retained trees."""
        if not os.path.exists(outputDir):
            os.makedirs(outputDir)
        for f in os.listdir(outputDir):
            os.remove(os.path.join(outputDir, f))
        files = self._treeFiles(geneTreeDir, extension)
        trees = []
        for f in files:
            with open(os.path.join(geneTreeDir, f)) as fin:
                root = parse_newick(fin.read())
            leaves, stack = [], [root]
            while stack:
                v = stack.pop()
                stack.extend(v.children)
                if not v.children:
                    leaves.append(plain_name(v.name))
            outgroup = []
            for label in leaves:
                g = genomeIdOfLabel(label)
                if g not in metadata:
                    raise ValueError('GeneTrees: tree %s has the leaf %s, whose genome %s has no metadata' % (f, label, g))
                if metadata[g]['taxonomy'][0].lower() == 'archaea':
                    outgroup.append(label)
            trees.append((f, GenomeTree.reroot(root, outgroup)))
        res = self.treeTests(trees, metadata, genomeIdOfGene)
        self.lastInfo = res['info']
        records = []
        for k, f in enumerate(files):
            p = res['packed'][k]
            paralogs, nonConspecific, at = [], [], 0
            for gi, pairs in enumerate(p.pairs):
                if res['pair_flag'][k][at:at + len(pairs)].any():
                    paralogs.append(p.genomes[p.groups[gi]])
                    if res['group_mixed'][k][gi]:
                        nonConspecific.append(p.genomes[p.groups[gi]])
                at += len(pairs)
            retained = not len(nonConspecific) > acceptPer * len(p.labels)
            if retained:
                shutil.copyfile(os.path.join(geneTreeDir, f), os.path.join(outputDir, f))
            records.append({'geneId': f[0:f.find('.')], 'numTaxa': len(p.labels), 'paralogs': sorted(paralogs), 'nonConspecific': sorted(nonConspecific), 'retained': retained})
        return records

    # ---- consistencyTest.py:53-253 ----------------------------------------------------------------------------------------------------
    @staticmethod
    def readDescriptions(tigrfamInfoDir, pfamClansFile):
        """{accession: [short, long]} (consistencyTest.py:63-86) from a directory of TIGRFAM INFO files and the Pfam-A.clans.tsv table."""
        descDict, acc = {}, None
        for f in sorted(os.listdir(tigrfamInfoDir)):
            shortDesc = longDesc = ''
            with open(os.path.join(tigrfamInfoDir, f)) as fin:
                for line in fin:
                    lineSplit = line.split('  ')
                    if lineSplit[0] == 'AC':
                        acc = lineSplit[1].strip()
                    elif lineSplit[0] == 'DE':
                        shortDesc = lineSplit[1].strip()
                    elif lineSplit[0] == 'CC':
                        longDesc = lineSplit[1].strip()
            if acc is not None:
                descDict[acc] = [shortDesc, longDesc]
        with open(pfamClansFile) as fin:
            for line in fin:
                lineSplit = line.split('\t')
                descDict[lineSplit[0]] = [lineSplit[3], lineSplit[4].strip()]
        return descDict

    def consistencyTest(self, geneTreeDir, metadata, descriptions, consistencyThreshold=0.86, minTaxaForAverage=20, extension='.tre', outputFile='./consistency.tsv',
                        outputDir='./data/gene_trees_final/'):
        """Writes <outputDir>/consistency/<tree>.results.tsv per tree and the combined table outputFile, copies the trees whose average
        consistency reaches the threshold into outputDir (whose files are removed first) and returns {tree file: [domain, phylum, class
        dictionaries taxon -> consistency or 'N/A']}."""
        if not os.path.exists(outputDir):
            os.makedirs(outputDir)
        for f in os.listdir(outputDir):
            if os.path.isfile(os.path.join(outputDir, f)):
                os.remove(os.path.join(outputDir, f))
        files = self._treeFiles(geneTreeDir, extension)
        trees = []
        for f in files:
            with open(os.path.join(geneTreeDir, f)) as fin:
                trees.append((f, fin.read()))
        res = self.treeTests(trees, metadata, genomeIdOfLabel)
        self.lastInfo = res['info']
        allResults, allTaxa, taxaCounts, avgConsistency = {}, [set(), set(), set()], {}, {}
        consistencyDir = os.path.join(outputDir, 'consistency')
        for k, treeFile in enumerate(files):
            p = res['packed'][k]
            hasInternal = bool(p.internal.any())
            consistencyDict, at = [{}, {}, {}], 0
            for r in range(3):
                for c, taxa in enumerate(p.classes[r]):
                    value = float(res['consistency'][k][at])
                    at += 1
                    allTaxa[r].add(taxa)
                    if not hasInternal:
                        consistencyDict[r][taxa] = 0
                    elif p.totals[r][c] <= 1 or taxa == 'unclassified':
                        consistencyDict[r][taxa] = 'N/A'
                    else:
                        consistencyDict[r][taxa] = value if value > 0 else 0
            totals = [dict(zip(p.classes[r], p.totals[r])) for r in range(3)]
            taxaCounts[treeFile] = [len(p.labels), totals[0].get('Bacteria', 0), totals[0].get('Archaea', 0)]
            if not os.path.exists(consistencyDir):
                os.makedirs(consistencyDir)
            with open(os.path.join(consistencyDir, treeFile + '.results.tsv'), 'w') as fout:
                fout.write('Tree')
                for r in range(3):
                    for taxa in sorted(consistencyDict[r].keys()):
                        fout.write('\t' + taxa)
                fout.write('\n')
                fout.write(treeFile)
                for r in range(3):
                    for taxa in sorted(consistencyDict[r].keys()):
                        if consistencyDict[r][taxa] != 'N/A':
                            fout.write('\t%.2f' % (consistencyDict[r][taxa] * 100))
                        else:
                            fout.write('\tN/A')
            average = []
            for r in range(3):
                sumConsistency = []
                for taxa in consistencyDict[r]:
                    if totals[r][taxa] > minTaxaForAverage and consistencyDict[r][taxa] != 'N/A':
                        sumConsistency.append(consistencyDict[r][taxa])
                if len(sumConsistency) > 0:
                    average.append(sum(sumConsistency) / len(sumConsistency))
                else:
                    average.append(0)
            avgConsistency[treeFile] = average
            allResults[treeFile] = consistencyDict
        with open(outputFile, 'w') as fout:
            fout.write('Tree\tShort Desc.\tLong Desc.\tAlignment Length\t# Taxa\t# Bacteria\t# Archaea\tAvg. Consistency\tAvg. Domain Consistency\tAvg. Phylum Consistency\tAvg. Class Consistency')
            for r in range(3):
                for t in sorted(allTaxa[r]):
                    fout.write('\t' + t)
            fout.write('\n')
            for treeFile in sorted(allResults.keys()):
                consistencyDict = allResults[treeFile]
                treeId = treeFile[0:treeFile.find('.')].replace('pfam', 'PF')
                if treeId not in descriptions:
                    raise ValueError('GeneTrees: tree %s has no description under %s' % (treeFile, treeId))
                fout.write(treeId + '\t' + descriptions[treeId][0] + '\t' + descriptions[treeId][1])
                fout.write('\t' + str(taxaCounts[treeFile][0]) + '\t' + str(taxaCounts[treeFile][1]) + '\t' + str(taxaCounts[treeFile][2]))
                avgCon = 0
                for r in range(3):
                    avgCon += avgConsistency[treeFile][r]
                avgCon /= 3
                fout.write('\t' + str(avgCon))
                if avgCon >= consistencyThreshold:
                    shutil.copyfile(os.path.join(geneTreeDir, treeFile), os.path.join(outputDir, treeFile))
                for r in range(3):
                    fout.write('\t' + str(avgConsistency[treeFile][r]))
                for r in range(3):
                    for t in sorted(allTaxa[r]):
                        if t in consistencyDict[r] and consistencyDict[r][t] != 'N/A':
                            fout.write('\t%.2f' % (consistencyDict[r][t] * 100))
                        else:
                            fout.write('\tN/A')
                fout.write('\n')
        return allResults

    # ---- the three in the reference's order -------------------------------------------------------------------------------------------
    def run(self, alignDir, workDir, metadata, descriptions, extension='.aln.masked.faa', model='kimura', maxDist=3.0, acceptPer=0.01, consistencyThreshold=0.86,
            minTaxaForAverage=20):
        """Trees, then the paralog test, then the consistency test, under workDir: gene_trees, gene_trees_conspecific, gene_trees_final and
        consistency.tsv.  Returns gene_trees_final, the directory GenomeTree.run takes as geneTreeDir."""
        treeDir, conspecificDir, finalDir = (os.path.join(workDir, d) for d in ('gene_trees', 'gene_trees_conspecific', 'gene_trees_final'))
        self.makeTrees(alignDir, treeDir, extension, model, maxDist)
        self.paralogTest(treeDir, metadata, acceptPer, '.tre', conspecificDir)
        self.consistencyTest(conspecificDir, metadata, descriptions, consistencyThreshold, minTaxaForAverage, '.tre', os.path.join(workDir, 'consistency.tsv'), finalDir)
        return finalDir
