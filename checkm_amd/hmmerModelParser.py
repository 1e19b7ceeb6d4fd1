"""Header view of HMMER3 profiles, API-compatible with checkm/hmmerModelParser.py:27-83.

`HmmModel` objects carry name/acc/leng/ga/tc/nc and pickle like the reference's
(checkm/markerSets.py:524-540).  The reference's header skim never resets its key dict between
records (hmmerModelParser.py:56), so ACC/GA/TC/NC of one record leak into following records that
lack them; `sticky_models` reproduces exactly that from the library's raw per-record headers.
"""


class HmmModelError(Exception):
    pass


class HmmModel(object):
    """Threshold/header view of one profile."""

    def __init__(self, keys):
        self.ga = None
        self.tc = None
        self.nc = None
        if 'acc' not in keys:
            self.acc = keys['name']
        for k, v in keys.items():
            setattr(self, k, v)


def sticky_models(headers):
    """headers: raw per-record dicts (name, acc|None, leng, ga|None, tc|None, nc|None), file order.
    Yields HmmModel with the carry-over of hmmerModelParser.py:56-81."""
    carried = {}
    for hd in headers:
        carried['format'] = 'HMMER3/f'
        carried['name'] = hd['name']
        if hd.get('acc') is not None:
            carried['acc'] = hd['acc']
        carried['leng'] = int(hd['leng'])
        for t in ('ga', 'tc', 'nc'):
            if hd.get(t) is not None:
                carried[t] = (float(hd[t][0]), float(hd[t][1]))
        yield HmmModel(dict(carried))


def models_dict(headers):
    """{acc: HmmModel} keyed the way HmmModelParser.models() keys it (hmmerModelParser.py:46-52)."""
    out = {}
    for m in sticky_models(headers):
        out[m.acc] = m
    return out


def read_headers(hmm_file):
    """Raw header records of a HMMER3 text file (host-side text skim; no scores are read here)."""
    headers = []
    cur = None
    in_body = False
    with open(hmm_file) as f:
        for line in f:
            if in_body:
                if line.startswith('//'):
                    headers.append(cur)
                    cur, in_body = None, False
                continue
            if line.startswith('HMMER'):
                cur = {'name': None, 'acc': None, 'leng': None, 'ga': None, 'tc': None, 'nc': None}
            elif line.startswith('HMM'):
                in_body = True
            else:
                fields = line.rstrip().split(None, 1)
                if len(fields) != 2:
                    raise HmmModelError("malformed header line: %r" % line)
                tag, val = fields
                if cur is None:
                    raise HmmModelError("header line outside a record: %r" % line)
                if tag == 'NAME':
                    cur['name'] = val
                elif tag == 'ACC':
                    cur['acc'] = val
                elif tag == 'LENG':
                    cur['leng'] = int(val)
                elif tag in ('GA', 'TC', 'NC'):
                    p = val.split()
                    if len(p) != 2:
                        raise HmmModelError("malformed %s line" % tag)
                    cur[tag.lower()] = (float(p[0].replace(';', '')), float(p[1].replace(';', '')))
    return headers


class HmmModelParser(object):
    """Drop-in for checkm.hmmerModelParser.HmmModelParser (header view only)."""

    def __init__(self, hmmFile):
        self.hmmFile = hmmFile
        self._headers = read_headers(hmmFile)

    def models(self):
        return models_dict(self._headers)

    def simpleParse(self):
        return sticky_models(self._headers)

    def parse(self):
        return sticky_models(self._headers)


# ---- nucleotide models (ALPH DNA / RNA): the integer tables of the SSU_Finder scan (checkm_amd/csrc/nhmm_dev.h) ---------------
NUC_FLOOR = -(1 << 21)        # what '*' (probability 0) becomes; nhmm_dev.h: FLOOR
NUC_MAX_M = 2048


def _lround(x):
    """C's lround: halves away from zero."""
    import math
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _millibits(field, offset_bits, top):
    """A -ln p field of the file as int32 milli-bits of log2(p) + offset_bits, inside [NUC_FLOOR, top]."""
    import math
    if field == '*':
        return NUC_FLOOR
    return max(NUC_FLOOR, min(top, _lround(1000.0 * (-float(field) / math.log(2.0) + offset_bits))))


class NucModel(object):
    """One nucleotide profile as the scan takes it: name, M (LENG), maxl (MAXL, or 2 M when the file has none), mu and lam of STATS LOCAL
    VITERBI, emis [4, M] (A C G T/U against the uniform background: log2(p / 0.25)) and trans [7, M] in the order MM IM DM MI II MD DD,
    node k at index k - 1, the transitions into k (MM IM DM MD DD) holding node k - 1's numbers and NUC_FLOOR at k = 1."""

    def __init__(self, name, M, maxl, mu, lam, emis, trans):
        self.name, self.M, self.maxl, self.mu, self.lam, self.emis, self.trans = name, M, maxl, mu, lam, emis, trans


def read_nuc_models(hmm_file):
    """Every ALPH DNA / RNA record of a HMMER3 text file as a NucModel.  Raises HmmModelError for another alphabet, a record without
    LENG or STATS LOCAL VITERBI, a malformed body, or more than 2048 nodes."""
    import numpy as np
    models = []
    with open(hmm_file) as f:
        lines = [ln.rstrip('\n') for ln in f]
    at = 0
    while at < len(lines):
        if not lines[at].startswith('HMMER3'):
            if lines[at].strip():
                raise HmmModelError("%s: line %d is outside a record" % (hmm_file, at + 1))
            at += 1
            continue
        at += 1
        name, M, maxl, alph, mu, lam = None, None, None, None, None, None
        while at < len(lines) and not lines[at].startswith('HMM '):
            w = lines[at].split()
            if w[:1] == ['NAME'] and len(w) > 1:
                name = w[1]
            elif w[:1] == ['LENG'] and len(w) > 1:
                M = int(w[1])
            elif w[:1] == ['MAXL'] and len(w) > 1:
                maxl = int(w[1])
            elif w[:1] == ['ALPH'] and len(w) > 1:
                alph = w[1].upper()
            elif w[:3] == ['STATS', 'LOCAL', 'VITERBI'] and len(w) >= 5:
                mu, lam = float(w[3]), float(w[4])
            at += 1
        if alph not in ('DNA', 'RNA'):
            raise HmmModelError("%s: model %s has alphabet %s, a nucleotide model has ALPH DNA or RNA" % (hmm_file, name, alph))
        if M is None or M < 1 or mu is None or at >= len(lines):
            raise HmmModelError("%s: model %s lacks LENG, STATS LOCAL VITERBI or its body" % (hmm_file, name))
        if M > NUC_MAX_M:
            raise HmmModelError("%s: model %s has %d nodes, the scan holds %d" % (hmm_file, name, M, NUC_MAX_M))
        at += 2                                                   # the two header lines of the body
        if at < len(lines) and lines[at].split()[:1] == ['COMPO']:
            at += 1
        node_t = []                                               # the seven transition fields of nodes 0 .. M
        match = []
        try:
            for k in range(M + 1):
                if k:
                    w = lines[at].split()
                    if int(w[0]) != k or len(w) < 5:
                        raise ValueError("match line of node %d" % k)
                    match.append(w[1:5])
                    at += 1
                if len(lines[at].split()) != 4:
                    raise ValueError("insert line of node %d" % k)
                w = lines[at + 1].split()
                if len(w) != 7:
                    raise ValueError("transition line of node %d" % k)
                node_t.append(w)
                at += 2
            if not lines[at].startswith('//'):
                raise ValueError("no // after node %d" % M)
            at += 1
        except (IndexError, ValueError) as e:
            raise HmmModelError("%s: model %s: malformed body (%s)" % (hmm_file, name, e))
        emis = np.array([[_millibits(match[k][c], 2.0, 2000) for k in range(M)] for c in range(4)], dtype=np.int32)
        trans = np.full((7, M), NUC_FLOOR, dtype=np.int32)
        MM, MI, MD, IM, II, DM, DD = range(7)                     # the file's column order
        for k in range(1, M + 1):
            trans[3, k - 1] = _millibits(node_t[k][MI], 0.0, 0)
            trans[4, k - 1] = _millibits(node_t[k][II], 0.0, 0)
            if k > 1:
                for row, col in ((0, MM), (1, IM), (2, DM), (5, MD), (6, DD)):
                    trans[row, k - 1] = _millibits(node_t[k - 1][col], 0.0, 0)
        models.append(NucModel(name, M, maxl if maxl is not None else 2 * M, mu, lam, emis, trans))
    return models
