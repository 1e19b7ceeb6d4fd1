"""Placement of bins in the reference genome tree: the step of `checkm tree` that the reference hands to the external programs pplacer and
guppy (checkm/pplacer.py).  `PplacerRunner.run` keeps the reference's files and `_createConcatenatedAlignment` its content; the
placement itself is a grid search on the device (checkm_amd/csrc/place_dev.h, kernels_place.hip): two Felsenstein sweeps per
chunk of sites, a scan of every (query, edge) at the edge's midpoint, and the caller's grid of distal fractions x pendant lengths on the
kept edges.  The host side here does every exp and log: the eigen-decomposition of the rate matrix, the tables of exp(lambda * rate * t)
the device multiplies with, one log per reported likelihood, the weight ratios, the .jplace file and the tree with the bins inserted
(`guppy tog`).  No external program is looked for or run.

Declared deviations from pplacer: a grid instead of Brent's optimiser; B, Z and every other character beyond the twenty
letters count as unknown; the substitution model is supplied by the user as a PAML .dat file with explicit rate categories; the four
named defaults are pplacer's as remembered, not checked against the program; no posterior-probability mode; no pre-masking.
"""
import json
import logging
import math
import os
import shutil
import stat
from collections import defaultdict

import numpy as np

from . import _lib, runtime
from .defaultValues import DefaultValues

STATES = 'ARNDCQEGHILKMFPSTWYV'          # PAML order
LN2 = math.log(2.0)
DEFAULT_PENDANT_GRID = tuple(float(x) for x in np.geomspace(1e-3, 2.0, 16))
DEFAULT_DISTAL_FRACTIONS = tuple((2 * k + 1) / 16.0 for k in range(8))


def discrete_gamma(alpha, ncat):
    """Mean-of-category rates of a discrete gamma distribution with shape alpha and mean 1 (Yang 1994), and equal weights."""
    from scipy.special import gammainc, gammaincinv
    cuts = gammaincinv(alpha, np.arange(1, ncat) / float(ncat))                 # quantiles of Gamma(alpha, 1)
    upper = np.concatenate([[0.0], gammainc(alpha + 1.0, cuts), [1.0]])         # integral of x f(x) up to a cut is alpha * I(alpha + 1, cut)
    return np.diff(upper) * ncat, np.full(ncat, 1.0 / ncat)


def read_paml_dat(path):
    """190 exchangeabilities (lower triangle, row by row) and 20 frequencies from a PAML .dat file -> (S [20, 20] symmetric, pi [20])."""
    nums = []
    with open(path) as f:
        for line in f:
            for tok in line.replace(',', ' ').split():
                try:
                    nums.append(float(tok))
                except ValueError:
                    break                                                      # the trailing prose of the PAML files
            if len(nums) >= 210:
                break
    if len(nums) < 210:
        raise ValueError('%s holds %d numbers, a PAML .dat holds 190 exchangeabilities and 20 frequencies' % (path, len(nums)))
    S = np.zeros((20, 20))
    k = 0
    for i in range(1, 20):
        for j in range(i):
            S[i, j] = S[j, i] = nums[k]
            k += 1
    pi = np.array(nums[190:210])
    return S, pi / pi.sum()


def eigen_model(S, pi):
    """U, Uinv, lambda of the reversible rate matrix Q_ij = S_ij pi_j scaled to one substitution per unit time: numpy.linalg.eigh on
    the symmetrised matrix, so that P(t) = U diag(exp(lambda t)) Uinv."""
    Q = S * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    Q = Q / -(pi * np.diag(Q)).sum()
    r = np.sqrt(pi)
    B = Q * r[:, None] / r[None, :]
    lam, V = np.linalg.eigh((B + B.T) / 2.0)
    return V / r[:, None], V.T * r[None, :], lam


# ---- the tree as written: labels, lengths and quoting kept ----------------------------------------------------------------------------------
class PNode(object):
    __slots__ = ('children', 'parent', 'name', 'length', 'num')

    def __init__(self):
        self.children, self.parent, self.name, self.length, self.num = [], None, '', None, -1


def parse_newick(text):
    """The root of one Newick statement.  A node keeps its name and its length as the text spells them (quotes included); [comments]
    and {edge numbers} are dropped.  Nodes are numbered as they close (jplace: a post-order walk of the tree as written)."""
    root = cur = PNode()
    i, n, count = 0, len(text), 0
    closed = False
    while i < n:
        c = text[i]
        if c.isspace():
            i += 1
        elif c == '[':
            i = text.index(']', i) + 1
        elif c == '{':
            i = text.index('}', i) + 1
        elif c == '(':
            child = PNode()
            child.parent = cur
            cur.children.append(child)
            cur = child
            i += 1
        elif c == ',' or c == ')':
            if cur.parent is None:
                raise ValueError('unbalanced parentheses in the tree')
            cur.num = count
            count += 1
            if c == ',':
                sib = PNode()
                sib.parent = cur.parent
                cur.parent.children.append(sib)
                cur = sib
            else:
                cur = cur.parent
            i += 1
        elif c == ':':
            j = i + 1
            while j < n and (text[j] in '+-.eE' or text[j].isdigit()):
                j += 1
            cur.length = text[i + 1:j]
            i = j
        elif c == ';':
            closed = True
            break
        elif c == "'":
            j = i + 1
            while True:
                j = text.index("'", j)
                if text[j + 1:j + 2] == "'":
                    j += 2
                    continue
                break
            cur.name = text[i:j + 1]
            i = j + 1
        else:
            j = i
            while j < n and text[j] not in '(),:;[{' and not text[j].isspace():
                j += 1
            cur.name = text[i:j]
            i = j
    if cur is not root or not root.children or not closed:
        raise ValueError('the tree is not one complete Newick statement')
    root.num = count
    return root


def plain_name(name):
    return name[1:-1].replace("''", "'") if name.startswith("'") else name


def nodes_of(root):
    """All nodes by number (post-order; the root last)."""
    out, stack = [], [root]
    while stack:
        v = stack.pop()
        out.append(v)
        stack.extend(v.children)
    return sorted(out, key=lambda v: v.num)


def quote_name(name):
    if name and all(ch.isalnum() or ch in '_.-|' for ch in name):
        return name
    return "'" + name.replace("'", "''") + "'"


def write_newick(root, inserts=None, edge_numbers=False):
    """The tree as text.  inserts: edge number -> [(name, distal, pendant)]: each query goes in on a node of its own, distal from the
    child end (guppy tog); several on one edge in order of distal length, then name.  edge_numbers: {n} after every length (jplace)."""
    inserts = inserts or {}

    def fmt(x):
        return repr(float(x))

    def render(v):
        body = '(' + ','.join(render(c) for c in v.children) + ')' + v.name if v.children else v.name
        if v.parent is None:
            return body
        here = sorted(inserts.get(v.num, ()), key=lambda t: (t[1], t[0]))
        if not here:
            tail = ':' + v.length if v.length is not None else (':0.0' if edge_numbers else '')
            return body + tail + ('{%d}' % v.num if edge_numbers else '')
        total = float(v.length) if v.length is not None else 0.0
        at = 0.0
        for name, distal, pendant in here:
            distal = min(max(distal, at), total)
            body = '(' + body + ':' + fmt(distal - at) + ',' + quote_name(name) + ':' + fmt(pendant) + ')'
            at = distal
        return body + ':' + fmt(total - at)

    return render(root) + ';'


class RefPkg(object):
    """A reference package as placement needs it: the tree, the aligned reference sequences and the model."""

    def __init__(self, tree_text, alignment, S, pi, rates=(1.0,), weights=None):
        self.root = parse_newick(tree_text)
        self.nodes = nodes_of(self.root)
        self.alignment = dict(alignment)
        self.rates = np.asarray(rates, dtype=np.float64).reshape(-1)
        self.weights = np.full(self.rates.shape[0], 1.0 / self.rates.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if self.rates.shape != self.weights.shape or not 1 <= self.rates.shape[0] <= 8:
            raise ValueError('1 to 8 rate categories, one weight each')
        self.pi = np.asarray(pi, dtype=np.float64)
        self.U, self.Uinv, self.lam = eigen_model(np.asarray(S, dtype=np.float64), self.pi)
        leaves = [v for v in self.nodes if not v.children]
        missing = [plain_name(v.name) for v in leaves if plain_name(v.name) not in self.alignment]
        if missing:
            raise ValueError('no aligned sequence for the leaves %s' % ', '.join(missing[:5]))
        self.nsites = len(self.alignment[plain_name(leaves[0].name)])

    @classmethod
    def from_dir(cls, path, model_file, rates=(1.0,), weights=None):
        """A pplacer reference package directory: CONTENTS.json names the Newick tree ('tree') and the aligned FASTA ('aln_fasta').
        The model comes from model_file, a PAML .dat (the package's own statistics file is not read)."""
        with open(os.path.join(path, 'CONTENTS.json')) as f:
            files = json.load(f)['files']
        with open(os.path.join(path, files['tree'])) as f:
            tree_text = f.read()
        S, pi = read_paml_dat(model_file)
        return cls(tree_text, read_fasta(os.path.join(path, files['aln_fasta'])), S, pi, rates, weights)


def read_fasta(path):
    seqs, cur = {}, None
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            if line[0] == '>':
                cur = line[1:].split(None, 1)[0]
                seqs[cur] = []
            else:
                seqs[cur].append(line.rstrip('\n'))
    return {k: ''.join(v) for k, v in seqs.items()}


def log_likelihood(m, e):
    """log(m * 2^e): the one log of a reported number."""
    return math.log(m) + e * LN2 if m > 0.0 else float('-inf')


class PplacerRunner(object):
    """Places bins in the reference genome tree on the device (the reference's class runs pplacer and guppy)."""

    def __init__(self, threads=1, modelFile=None, rates=(1.0,), weights=None):
        self.logger = logging.getLogger('timestamp')
        self.numThreads = threads
        self.modelFile = modelFile or os.environ.get('CKM_PLACE_MODEL')
        self.rates, self.weights = rates, weights

    # ---- checkm tree -----------------------------------------------------------------------------------------------------------------
    def run(self, binFiles, resultsParser, outDir, bReducedTree):
        alignOutputDir = os.path.join(outDir, 'storage', 'tree')
        os.makedirs(alignOutputDir, exist_ok=True)
        treeFile = os.path.join(alignOutputDir, DefaultValues.PPLACER_TREE_OUT)
        pplacerJsonOut = os.path.join(alignOutputDir, DefaultValues.PPLACER_JSON_OUT)
        pplacerOut = os.path.join(alignOutputDir, DefaultValues.PPLACER_OUT)
        concatenatedAlignFile = self._createConcatenatedAlignment(binFiles, resultsParser, alignOutputDir)
        pplacerRefPkg = DefaultValues.PPLACER_REF_PACKAGE_REDUCED if bReducedTree else DefaultValues.PPLACER_REF_PACKAGE_FULL
        if os.stat(concatenatedAlignFile)[stat.ST_SIZE] == 0:
            self.logger.info('No genomes were identified that could be placed in the reference genome tree.')
            shutil.copyfile(os.path.join(pplacerRefPkg, DefaultValues.GENOME_TREE), treeFile)
            return
        if not self.modelFile:
            raise ValueError('placement needs the substitution model of the reference package as a PAML .dat file: PplacerRunner(threads, modelFile=...) or CKM_PLACE_MODEL')
        self.logger.info('Placing %d bins into the genome tree on the device.' % len(binFiles))
        refpkg = RefPkg.from_dir(pplacerRefPkg, self.modelFile, self.rates, self.weights)
        queries = read_fasta(concatenatedAlignFile)
        placements, info = self.place(refpkg, queries, withInfo=True)
        self.writeJplace(refpkg, placements, pplacerJsonOut)
        with open(pplacerOut, 'w') as f:
            f.write('checkm_amd placement: %d queries, %d edges, %d sites, %d rate categories\n' % (len(queries), len(refpkg.nodes) - 1, refpkg.nsites, refpkg.rates.shape[0]))
            f.write('chunks %d of %d sites, %.1f ms\n' % (info['nchunks'], info['chunk_sites'], info['ms_total']))
        with open(treeFile, 'w') as f:
            f.write(self.tog(refpkg, placements) + '\n')

    def _createConcatenatedAlignment(self, binFiles, resultsParser, alignOutputDir):
        """Create a concatenated alignment of marker genes for each bin (checkm/pplacer.py:89-132).  The reference writes the records
        in the order of a set of bin ids; here they go in sorted order."""
        self.logger.info('Reading marker alignment files.')
        alignments = defaultdict(dict)
        binIds = set()
        for f in os.listdir(alignOutputDir):
            if f.endswith('.masked.faa'):
                markerId = f[0:f.find('.masked.faa')]
                for seqId, seq in read_fasta(os.path.join(alignOutputDir, f)).items():
                    binId = seqId[0:seqId.find(DefaultValues.SEQ_CONCAT_CHAR)]
                    alignments[markerId][binId] = seq
                    binIds.add(binId)
        models = resultsParser.models[list(resultsParser.models.keys())[0]]
        self.logger.info('Concatenating alignments.')
        concatenatedSeqs = {}
        for markerId in sorted(models.keys()):
            seqs = alignments[markerId]
            for binId in binIds:
                concatenatedSeqs[binId] = concatenatedSeqs.get(binId, '') + (seqs[binId] if binId in seqs else '-' * models[markerId].leng)
        concatenatedAlignFile = os.path.join(alignOutputDir, DefaultValues.PPLACER_CONCAT_SEQ_OUT)
        with open(concatenatedAlignFile, 'w') as fout:
            for binId in sorted(concatenatedSeqs):
                fout.write('>' + binId + '\n')
                fout.write(concatenatedSeqs[binId] + '\n')
        return concatenatedAlignFile

    # ---- placement -------------------------------------------------------------------------------------------------------------------
    def _tables(self, refpkg, queries, pendantGrid=None, distalFractions=None, startPend=0.1, maxPitches=40):
        """The arrays of the device call: the tree by jplace edge numbers, the alignment rows of the leaves, the queries in sorted
        order of their names, and the tables of exp(lambda * rate * t) for every t the device needs."""
        pend = np.asarray(DEFAULT_PENDANT_GRID if pendantGrid is None else pendantGrid, dtype=np.float64).reshape(-1)
        frac = np.asarray(DEFAULT_DISTAL_FRACTIONS if distalFractions is None else distalFractions, dtype=np.float64).reshape(-1)
        names = sorted(queries)
        bad = [q for q in names if len(queries[q]) != refpkg.nsites]
        if bad:
            raise ValueError('query %s has %d columns, the reference alignment %d' % (bad[0], len(queries[bad[0]]), refpkg.nsites))
        nodes = refpkg.nodes
        child_off = np.zeros(len(nodes) + 1, dtype=np.uint64)
        child = []
        for v in nodes:
            child.extend(c.num for c in v.children)
            child_off[v.num + 1] = len(child)
        length = np.array([float(v.length) if v.length is not None and v.parent is not None else 0.0 for v in nodes])
        rows = [refpkg.alignment[plain_name(v.name)].encode('latin-1') for v in nodes if not v.children]
        qs = [queries[q].encode('latin-1') for q in names]
        off = lambda seqs: np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        lr = refpkg.lam[None, :] * refpkg.rates[:, None]                        # [R, 20]
        table = lambda t: np.exp(lr * np.asarray(t, dtype=np.float64)[..., None, None])
        dist = np.stack([length[:, None] * frac[None, :], length[:, None] * (1.0 - frac)[None, :]], axis=2)      # [N, F, 2]
        t = _lib.PlaceTables(child_off, child, length, refpkg.nsites, off(rows), b''.join(rows), off(qs), b''.join(qs), refpkg.weights, refpkg.U, refpkg.Uinv,
                             refpkg.pi, table(length), table(length / 2.0), table(dist), table(np.concatenate([[startPend], pend])), maxPitches)
        t.names, t.pend, t.frac = names, pend, frac
        return t

    @staticmethod
    def _placements(tables, res, keepAtMost=7, keepFactor=0.01):
        """name -> the kept placements (edge_num, logL, like_weight_ratio, distal_length, pendant_length), best first."""
        out = {}
        for qi, name in enumerate(tables.names):
            rows = []
            for k in range(res['top_edge'].shape[1]):
                e = int(res['top_edge'][qi, k])
                if e < 0:
                    break
                rows.append((e, log_likelihood(float(res['ref_m'][qi, k]), int(res['ref_e'][qi, k])), float(tables.frac[res['ref_f'][qi, k]] * tables.length[e]),
                             float(tables.pend[res['ref_g'][qi, k]])))
            rows.sort(key=lambda r: (-r[1], r[0]))
            top = rows[0][1] if rows else 0.0
            total = top + math.log(sum(math.exp(r[1] - top) for r in rows)) if rows and top > float('-inf') else float('-inf')
            ratio = [math.exp(r[1] - total) if total > float('-inf') else 1.0 / len(rows) for r in rows]
            out[name] = [(r[0], r[1], w, r[2], r[3]) for r, w in list(zip(rows, ratio))[:keepAtMost] if w >= keepFactor * ratio[0]]
        return out

    def place(self, refpkg, queries, pendantGrid=None, distalFractions=None, startPend=0.1, maxPitches=40, keepAtMost=7, keepFactor=0.01, budget_bytes=0, withInfo=False):
        """Place `queries` ({name: aligned sequence}) on the edges of refpkg's tree.  Returns name -> kept placements, each
        (edge_num, logL, like_weight_ratio, distal_length, pendant_length), best first."""
        tables = self._tables(refpkg, queries, pendantGrid, distalFractions, startPend, maxPitches)
        res = _lib.place_run(runtime.get_ctx(), tables, budget_bytes)
        placements = self._placements(tables, res, keepAtMost, keepFactor)
        return (placements, res) if withInfo else placements

    # ---- outputs ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def tog(refpkg, placements):
        """The reference tree with every query inserted at its best placement (guppy tog)."""
        inserts = defaultdict(list)
        for name, rows in placements.items():
            if rows:
                inserts[rows[0][0]].append((name, rows[0][3], rows[0][4]))
        return write_newick(refpkg.root, inserts)

    @staticmethod
    def writeJplace(refpkg, placements, path):
        doc = {'tree': write_newick(refpkg.root, edge_numbers=True),
               'placements': [{'p': [[r[0], r[1], r[2], r[3], r[4]] for r in rows], 'n': [name]} for name, rows in sorted(placements.items())],
               'metadata': {'invocation': 'checkm_amd.pplacer'}, 'version': 3,
               'fields': ['edge_num', 'likelihood', 'like_weight_ratio', 'distal_length', 'pendant_length']}
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
