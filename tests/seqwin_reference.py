"""TEST INFRASTRUCTURE: a plain-Python restatement of the per-window numbers of CheckM's plot commands (checkm/plot/gcPlots.py:55-75,
gcBiasPlots.py:51-66, codingDensityPlots.py:73-89, tetraDistPlots.py:63-79): slices and str.count, a dict of 4-mers, a numpy mask.
tests/test_seqwin_host.py pins it to what the reference's own plot classes hand to their axes (tests/golden/seqwin_cases.json)."""
import numpy as np

_COMPL = str.maketrans("ACGT", "TGCA")
_MERS = [a + b + c + d for a in "ACGT" for b in "ACGT" for c in "ACGT" for d in "ACGT"]
_COLS = sorted(set(min(m, m.translate(_COMPL)[::-1]) for m in _MERS))
KMER_INDEX = {m: _COLS.index(min(m, m.translate(_COMPL)[::-1])) for m in _MERS}


def read_fasta(text):
    """{id: sequence} of a FASTA text without blank lines, every line ended by a newline (what the fixtures hold)."""
    seqs, cur = {}, None
    for line in text.splitlines():
        if line.startswith(">"):
            cur = line[1:].split(None, 1)[0]
            seqs[cur] = []
        else:
            seqs[cur].append(line)
    return {k: "".join(v) for k, v in seqs.items()}


def base_count(seq):
    s = seq.upper()
    return s.count("A"), s.count("C"), s.count("G"), s.count("T") + s.count("U")


def windows(seq, w):
    """The slices the plot loops take: `while end < seqLen`."""
    out, start, end = [], 0, w
    while end < len(seq):
        out.append(seq[start:end])
        start = end
        end += w
    return out


def tetra_counts(seq):
    sig = [0] * 136
    s = seq.upper()
    for i in range(len(s) - 3):
        k = KMER_INDEX.get(s[i:i + 4])
        if k is not None:
            sig[k] += 1
    return sig


def signature(seq):
    sig = np.array(tetra_counts(seq), dtype=float)
    with np.errstate(invalid="ignore"):
        sig /= np.sum(sig)
    return sig


def distance(a, b):
    return np.sum(np.abs(a - b))


def bin_sig(seqs, tetraSigs):
    size = sum(len(s) for s in seqs.values())
    out = None
    for seqId, seq in seqs.items():
        weighted = tetraSigs[seqId] * (float(len(seq)) / size)
        if out is None:
            out = weighted
        else:
            out += weighted
    return out


def parse_gff(text):
    """({seqId: {geneId: [start, end]}}, {seqId: last coding base}) as ProdigalGeneFeatureParser._parseGFF keeps them."""
    genes, last, counter = {}, {}, 0
    for line in text.splitlines(True):
        if line[0] == "#" or line.strip() == '"':
            continue
        cols = line.split("\t")
        if cols[0] not in genes:
            counter = 0
            genes[cols[0]] = {}
            last[cols[0]] = 0
        genes[cols[0]][cols[0] + "_" + str(counter)] = [int(cols[3]), int(cols[4])]
        counter += 1
        last[cols[0]] = max(last[cols[0]], int(cols[4]))
    return genes, last


def coding_masks(gff_text):
    genes, last = parse_gff(gff_text)
    masks = {}
    for seqId in genes:
        m = np.zeros(last[seqId])
        for a, z in genes[seqId].values():
            m[a - 1:z] = 1
        masks[seqId] = m
    return masks


def gc_windows(seqs, w):
    data = []
    for seq in seqs.values():
        for win in windows(seq, w):
            a, c, g, t = base_count(win)
            if a + c + g + t:
                data.append(float(g + c) / (a + c + g + t))
    return data, [len(s) for s in seqs.values()]


def gc_profile(seqs, w):
    out = {}
    for seqId, seq in seqs.items():
        wins = []
        for win in windows(seq, w):
            a, c, g, t = base_count(win)
            wins.append(float(g + c) / (a + c + g + t))
        a, c, g, t = base_count(seq)
        out[seqId] = [float(g + c) / (a + c + g + t), wins]
    return out


def cd_windows(seqs, gff_text, w):
    masks = coding_masks(gff_text)
    data = []
    for seqId, seq in seqs.items():
        for k, win in enumerate(windows(seq, w)):
            coding = np.sum(masks[seqId][k * w:(k + 1) * w]) if seqId in masks else 0
            a, c, g, t = base_count(win)
            data.append(float(coding) / (a + c + g + t))
    return data, [len(s) for s in seqs.values()]


def td_windows(seqs, tetraSigs, w):
    b = bin_sig(seqs, tetraSigs)
    data, deltas = [], []
    for seqId, seq in seqs.items():
        deltas.append(distance(tetraSigs[seqId], b))
        for win in windows(seq, w):
            data.append(distance(signature(win), b))
    return data, [len(s) for s in seqs.values()], deltas


def hexes(values):
    return [float(v).hex() for v in values]
