"""TEST INFRASTRUCTURE: seeded nucleotide models in HMMER3 text form and contigs with planted, mutated copies for the SSU_Finder tests.
A model has a random consensus with probability 0.85 on the consensus base, plain transition probabilities, a MAXL line and STATS
LOCAL lines with a made-up mu and lambda = 0.693."""
import math
import os

import numpy as np

BASES = 'ACGT'
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N', 'a': 't', 'c': 'g', 'g': 'c', 't': 'a', 'n': 'n', 'U': 'A', 'u': 'a'}
T_NODE = (0.97, 0.015, 0.015, 0.6, 0.4, 0.6, 0.4)       # MM MI MD IM II DM DD


def revcomp(s):
    return ''.join(COMP.get(c, c) for c in reversed(s))


def _f(p):
    return '*' if p <= 0.0 else '%.5f' % (0.0 if p >= 1.0 else -math.log(p))


def _head(name, M, maxl, mu, lam, alph, with_maxl, with_compo):
    """The lines of a record down to the insert line of node 0, and the uniform emission line."""
    out = ['HMMER3/f [synthetic]', 'NAME  %s' % name, 'LENG  %d' % M]
    if with_maxl:
        out.append('MAXL  %d' % (maxl if maxl is not None else M + M // 4 + 8))
    out += ['ALPH  %s' % alph, 'RF    no', 'MM    no', 'CONS  yes', 'CS    no', 'MAP   no', 'NSEQ  1', 'EFFN  1.0',
            'STATS LOCAL MSV      %.4f  %.5f' % (mu - 1.0, lam), 'STATS LOCAL VITERBI  %.4f  %.5f' % (mu, lam), 'STATS LOCAL FORWARD  %.4f  %.5f' % (mu + 3.0, lam),
            'HMM          A        C        G        T   ', '            m->m     m->i     m->d     i->m     i->i     d->m     d->d']
    quarter = '  '.join([_f(0.25)] * 4)
    if with_compo:
        out.append('  COMPO   ' + quarter)
    out.append('          ' + quarter)
    return out, quarter


def _per_node_text(name, consensus, maxl, mu, lam, alph, with_maxl, with_compo, rng, star):
    M = len(consensus)
    match, trans = per_node_probs(rng, M, star)
    match_text, trans_text = [[_f(p) for p in row] for row in match], [[_f(p) for p in row] for row in trans]
    out, quarter = _head(name, M, maxl, mu, lam, alph, with_maxl, with_compo)
    out.append('          ' + '  '.join(trans_text[0]))
    for k in range(1, M + 1):
        out.append('%7d   %s %6d %s - - -' % (k, '  '.join(match_text[k - 1]), k, consensus[k - 1].lower()))
        out.append('          ' + quarter)
        out.append('          ' + '  '.join(trans_text[k]))
    out.append('//')
    return '\n'.join(out) + '\n', dict(match=match, trans=trans, match_text=match_text, trans_text=trans_text)


def per_node_probs(rng, M, star=0.0):
    """Probabilities of a model whose every node has its own numbers: match [M, 4] and trans [M + 1, 7] (nodes 0 .. M, the file's order
    MM MI MD IM II DM DD).  Each row of match, and each of MM MI MD / IM II / DM DD, sums to one before a share `star` of the entries is
    set to 0 (printed as '*'); the printed fields of a node's seven transitions and of its four emissions are pairwise distinct, '*'
    apart.  Node 0 and node M keep the file's fixed entries: DM = 1 and DD = 0, and at node M also MD = 0."""
    match, trans = np.zeros((M, 4)), np.zeros((M + 1, 7))
    for k in range(M + 1):
        while True:
            e = rng.dirichlet((1.0, 1.0, 1.0, 1.0))
            t = np.concatenate([rng.dirichlet((6.0, 1.0, 1.0)), rng.dirichlet((2.0, 1.0)), rng.dirichlet((2.0, 1.0))])
            if k == 0 or k == M:
                t[5:] = (1.0, 0.0)
            if k == M:
                t[:3] = (t[0] + t[2], t[1], 0.0)
            e[rng.random(4) < star] = 0.0
            t[:5][rng.random(5) < star] = 0.0
            if 0 < k < M:
                t[5:][rng.random(2) < star] = 0.0
            shown = [[_f(p) for p in v if 0.0 < p < 1.0] for v in (e, t)]
            if all(len(set(s)) == len(s) for s in shown):
                break
        trans[k] = t
        if k:
            match[k - 1] = e
    return match, trans


def model_text(name, consensus, maxl=None, mu=2.0, lam=0.693, alph='DNA', p_cons=0.85, t_node=T_NODE, with_maxl=True, with_compo=True, per_node=None, star=0.0):
    """The text of one model.  per_node = a numpy Generator: every node draws its own match emissions and transitions (per_node_probs,
    `star` the share of '*' entries), and the return value is (text, probs): probs['match'] [M, 4] and probs['trans'] [M + 1, 7] the
    probabilities, probs['match_text'] and probs['trans_text'] the fields as printed."""
    M = len(consensus)
    if per_node is not None:
        return _per_node_text(name, consensus, maxl, mu, lam, alph, with_maxl, with_compo, per_node, star)
    out, quarter = _head(name, M, maxl, mu, lam, alph, with_maxl, with_compo)
    out.append('          ' + '  '.join(_f(p) for p in (t_node[0], t_node[1], t_node[2], t_node[3], t_node[4], 1.0, 0.0)))
    rest = (1.0 - p_cons) / 3.0
    for k in range(1, M + 1):
        c = consensus[k - 1]
        out.append('%7d   %s %6d %s - - -' % (k, '  '.join(_f(p_cons if b == c else rest) for b in BASES), k, c.lower()))
        out.append('          ' + quarter)
        t = t_node if k < M else (t_node[0] + t_node[2], t_node[1], 0.0, t_node[3], t_node[4], 1.0, 0.0)
        out.append('          ' + '  '.join(_f(p) for p in t))
    out.append('//')
    return '\n'.join(out) + '\n'


def write_model(path, name, M, seed, **kw):
    """A seeded model file; returns its consensus, or with per_node=rng (model_text) the pair (consensus, probs)."""
    rng = np.random.default_rng(seed)
    consensus = ''.join(BASES[i] for i in rng.integers(0, 4, M))
    text = model_text(name, consensus, **kw)
    probs = None
    if kw.get('per_node') is not None:
        text, probs = text
    with open(path, 'w') as f:
        f.write(text)
    return consensus if probs is None else (consensus, probs)


def random_dna(rng, n):
    return ''.join(BASES[i] for i in rng.integers(0, 4, n))


def mutated_copy(rng, consensus, sub=0.10, ins=0.01, dele=0.01, clean=20):
    """A copy of the consensus whose first and last `clean` bases are exact; elsewhere substitutions, insertions and deletions."""
    out = []
    M = len(consensus)
    for k, c in enumerate(consensus):
        if k < clean or k >= M - clean:
            out.append(c)
            continue
        r = rng.random()
        if r < dele:
            continue
        if r < dele + sub:
            c = BASES[(BASES.index(c) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(c)
        if rng.random() < ins:
            out.append(BASES[int(rng.integers(0, 4))])
    return ''.join(out)


def planted_contig(rng, length, copies):
    """A random contig of about `length` bases with `copies` = [(position of the first base, 0-based, copy text, reverse?)] written over it.
    Returns (text, [(from, to, reverse)]) with 1-based closed forward coordinates."""
    s = list(random_dna(rng, length))
    where = []
    for at, text, rev in copies:
        t = revcomp(text) if rev else text
        s[at:at + len(t)] = list(t)
        where.append((at + 1, at + len(t), rev))
    return ''.join(s[:max(length, max([0] + [w[1] for w in where]))]), where


def write_fasta(path, records, width=70):
    import gzip
    op = gzip.open if path.endswith('.gz') else open
    with op(path, 'wt') as f:
        for name, seq in records:
            f.write('>%s\n' % name)
            for k in range(0, len(seq), width):
                f.write(seq[k:k + width] + '\n')
            if not seq:
                f.write('\n')


def data_dir(root, Ms=(120, 100, 90), seed=100):
    """A three-model data directory as DefaultValues.CHECKM_DATA_DIR/hmms_ssu; returns {domain: consensus}."""
    d = os.path.join(root, 'hmms_ssu')
    os.makedirs(d, exist_ok=True)
    return {dom: write_model(os.path.join(d, 'SSU_%s.hmm' % dom), 'SSU_' + dom, M, seed + k) for k, (dom, M) in enumerate(zip(('bacteria', 'archaea', 'euk'), Ms))}
