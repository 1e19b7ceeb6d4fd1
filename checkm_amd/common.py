"""Small helpers with the reference's semantics (checkm/common.py)."""
import ast
import errno
import os
import sys
import logging


def binIdFromFilename(filename):
    """Basename minus one compression suffix minus one extension."""
    binId = os.path.basename(filename)
    if binId.endswith('.gz'):
        binId = binId[0:-3]
    root, _ext = os.path.splitext(binId)
    return root


def makeSurePathExists(path):
    if not path:
        return
    try:
        os.makedirs(path)
    except OSError as e:
        if e.errno != errno.EEXIST:
            logging.getLogger('timestamp').error('Specified path could not be created: ' + path)
            sys.exit(1)


def getBinIdsFromOutDir(outDir):
    binIds = []
    binDir = os.path.join(outDir, 'bins')
    for f in os.listdir(binDir):
        if os.path.isdir(os.path.join(binDir, f)):
            binIds.append(f)
    return binIds


def checkFileExists(inputFile):
    if not os.path.exists(inputFile):
        logging.getLogger('timestamp').error('Input file does not exists: ' + inputFile)
        sys.exit(1)


def readDistribution(prefix):
    """The dict literal of <DISTRIBUTION_DIR>/<prefix>.txt (gc_dist, cd_dist, td_dist)."""
    from checkm_amd.defaultValues import DefaultValues
    distFile = os.path.join(DefaultValues.DISTRIBUTION_DIR, prefix + '.txt')
    checkFileExists(distFile)
    with open(distFile, 'r') as f:
        return ast.literal_eval(f.read())


def findNearest(array, value):
    """The element of array nearest to value; of two equally near ones the first (numpy's argmin)."""
    import numpy as np
    idx = (np.abs(np.array(array) - value)).argmin()
    return array[idx]


def read_fasta(path):
    """[(name, description, residues)] from a (optionally gzipped) FASTA file."""
    import gzip
    op = gzip.open if path.endswith('.gz') else open
    recs, name, desc, parts = [], None, '', []
    with op(path, 'rt') as f:
        for line in f:
            if not line:
                continue
            if line[0] == '>':
                if name is not None:
                    recs.append((name, desc, ''.join(parts)))
                hdr = line[1:].rstrip('\r\n')
                sp = hdr.split(None, 1)
                name = sp[0] if sp else ''
                desc = sp[1] if len(sp) > 1 else ''
                parts = []
            else:
                parts.append(line.strip())
    if name is not None:
        recs.append((name, desc, ''.join(parts)))
    return recs


def _centre(text, width):
    excess = width - len(text)
    left = excess // 2
    if excess % 2 and len(text) % 2 == 0:          # the odd blank goes left of a text of even length, right of an odd one
        left += 1
    return ' ' * left + text + ' ' * (excess - left)


def frame_table(header, rows, sort_col=None, reverse=False):
    """The framed table of the non-tab output modes (qa, profile), in the layout the reference's table writer produces for the settings
    it is given there: rules above the header, below it and at the end, no vertical rules, one blank of padding, the first column left,
    the others centred, floats as %.2f.  sort_col: rows ordered by that column, ties by the whole row (as a decorated sort does)."""
    rows = list(rows)
    if sort_col is not None:
        i = header.index(sort_col)
        rows.sort(key=lambda r: [r[i]] + list(r), reverse=reverse)
    cells = [[('%.2f' % v) if isinstance(v, float) else str(v) for v in row] for row in rows]
    width = [max([len(h)] + [len(r[k]) for r in cells]) for k, h in enumerate(header)]
    rule = '-' + ''.join('-' * (w + 3) for w in width)

    def line(values):
        return ' ' + ''.join(' ' + (v.ljust(w) if k == 0 else _centre(v, w)) + '  ' for k, (v, w) in enumerate(zip(values, width)))
    return '\n'.join([rule, line(header), rule] + [line(r) for r in cells] + [rule])
