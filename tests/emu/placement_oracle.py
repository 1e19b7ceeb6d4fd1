"""TEST INFRASTRUCTURE: a second formulation of the placement likelihood, independent of checkm_amd/csrc/place_dev.h: the query is actually
inserted in the tree (a new node on the edge, the query on a pendant edge), Felsenstein pruning runs from the leaves to the root of that
tree with numpy, and every P(t) is scipy.linalg.expm(Q * rate * t).  Slow and plain on purpose.  Also the helpers the tests and
tools/gen_placement_golden.py share: random trees, random reversible models, simulation of an alignment down a tree, pruning a leaf."""
import math

import numpy as np

from checkm_amd.pplacer import STATES, PNode, nodes_of, parse_newick, plain_name, write_newick


def rate_matrix(S, pi):
    """Q_ij = S_ij pi_j, rows summing to zero, one substitution per unit time."""
    Q = np.asarray(S, dtype=np.float64) * np.asarray(pi)[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q / -(np.asarray(pi) * np.diag(Q)).sum()


def tip(seq):
    """[sites, 20]: one-hot for the twenty upper-case letters, all ones for everything else."""
    out = np.ones((len(seq), 20))
    for s, ch in enumerate(seq):
        k = STATES.find(ch)
        if k >= 0:
            out[s] = 0.0
            out[s, k] = 1.0
    return out


class Oracle(object):
    def __init__(self, S, pi, rates, weights):
        self.Q, self.pi = rate_matrix(S, pi), np.asarray(pi, dtype=np.float64)
        self.rates, self.weights = [float(r) for r in rates], [float(w) for w in weights]
        self._P = {}

    def P(self, t, r):
        from scipy.linalg import expm
        key = (float(t), r)
        if key not in self._P:
            self._P[key] = expm(self.Q * (self.rates[r] * float(t)))
        return self._P[key]

    def log_likelihood(self, tree, seqs):
        """tree: nested tuples (children, name, length) with children a list (empty for a leaf); seqs: name -> sequence."""
        total = None
        for r, w in enumerate(self.weights):
            def partial(node):
                children, name, _length = node
                if not children:
                    return tip(seqs[name]), 0.0
                L, logs = None, 0.0
                for c in children:
                    Lc, lc = partial(c)
                    msg = Lc @ self.P(c[2], r).T
                    L = msg if L is None else L * msg
                    logs = logs + lc
                mx = L.max(axis=1)
                return L / mx[:, None], logs + np.log(mx)
            L, logs = partial(tree)
            site = np.log(L @ self.pi) + logs
            total = site + math.log(w) if total is None else np.logaddexp(total, site + math.log(w))
        return float(total.sum())

    def placed(self, root, alignment, query, edge, distal, pendant):
        """log-likelihood of the reference tree (a PNode root) with `query` attached on edge `edge`, `distal` from its child end."""
        def build(v):
            length = float(v.length) if v.length is not None and v.parent is not None else 0.0
            sub = ([build(c) for c in v.children], plain_name(v.name), length)
            if v.num != edge:
                return sub
            return ([(sub[0], sub[1], distal), ([], '\0query', pendant)], '', length - distal)
        seqs = dict(alignment)
        seqs['\0query'] = query
        return self.log_likelihood(build(root), seqs)


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------------
def random_model(rng):
    """A random reversible 20-state model: (S [20, 20] symmetric, pi)."""
    S = np.zeros((20, 20))
    iu = np.triu_indices(20, 1)
    S[iu] = rng.gamma(1.0, 1.0, size=190) + 0.05
    S = S + S.T
    pi = rng.dirichlet(np.full(20, 5.0))
    return S, pi


def random_tree(rng, nleaves, lo=0.08, hi=0.3, root_degree=3, prefix='t'):
    """Newick text of a random tree: leaves joined at random until root_degree subtrees are left."""
    parts = ['%s%d' % (prefix, k) for k in range(nleaves)]
    fmt = lambda: '%.6f' % rng.uniform(lo, hi)
    while len(parts) > root_degree:
        i, j = sorted(rng.choice(len(parts), size=2, replace=False).tolist())
        b = parts.pop(j)
        a = parts.pop(i)
        parts.append('(%s:%s,%s:%s)' % (a, fmt(), b, fmt()))
    return '(' + ','.join('%s:%s' % (p, fmt()) for p in parts) + ');'


def simulate(rng, root, S, pi, rates, weights, nsites):
    """name -> sequence: states drawn at the root from pi, a rate category per site, and down every edge by expm."""
    from scipy.linalg import expm
    Q = rate_matrix(S, pi)
    cat = rng.choice(len(rates), size=nsites, p=np.asarray(weights) / np.sum(weights))
    out = {}

    def walk(v, states):
        if not v.children:
            out[plain_name(v.name)] = ''.join(STATES[k] for k in states)
        for c in v.children:
            nxt = np.empty(nsites, dtype=np.int64)
            for r in range(len(rates)):
                P = expm(Q * rates[r] * float(c.length))
                P = np.clip(P, 0.0, None)
                P = P / P.sum(axis=1, keepdims=True)
                for s in np.nonzero(cat == r)[0]:
                    nxt[s] = rng.choice(20, p=P[states[s]])
            walk(c, nxt)

    walk(root, rng.choice(20, size=nsites, p=pi))
    return out


def prune_leaf(tree_text, leaf):
    """(Newick of the tree without `leaf`, the jplace edge numbers of that tree the leaf hung on).  The leaf's parent goes and its
    sibling's edge takes both lengths; under a root of three the two remaining root edges are one edge of the unrooted tree."""
    root = parse_newick(tree_text)
    v = [x for x in nodes_of(root) if not x.children and plain_name(x.name) == leaf][0]
    p = v.parent
    p.children.remove(v)
    marks = []
    if p.parent is None:
        if len(p.children) < 2:
            raise ValueError('the leaf hangs on a root of two')
        marks = list(p.children)
    elif len(p.children) == 1:
        sib = p.children[0]
        sib.length = '%.6f' % (float(sib.length) + float(p.length))
        sib.parent = p.parent
        p.parent.children[p.parent.children.index(p)] = sib
        marks = [sib]
    else:
        marks = [p]
    text = write_newick(root)
    again = parse_newick(text)
    key = lambda x: write_newick_sub(x)
    want = set(key(m) for m in marks)
    return text, sorted(x.num for x in nodes_of(again) if x.parent is not None and key(x) in want)


def write_newick_sub(v):
    return ('(' + ','.join(write_newick_sub(c) + ':' + str(c.length) for c in v.children) + ')' + v.name) if v.children else v.name
