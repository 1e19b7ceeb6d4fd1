"""Seeded synthetic alignments for ReducedTree: the tests, tools/reducedtree_bench.py and the --time run of tools/gen_reducedtree_golden.py
draw from the same generator, so that their figures speak of the same composition."""
import numpy as np

LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY-", dtype=np.uint8)


def alignment(seed, rows, columns, clade=50, clade_rate=0.3, group=4, group_every=10, max_diff_perc=0.08):
    """[rows, columns] uint8.  Rows come in clades of `clade`: each row is its clade's ancestor with a fraction clade_rate of its columns
    redrawn (so rows of one clade differ in about 1 - (1 - rate)^2 of the columns, rows of two clades in about 20 of 21).  Every
    group_every-th row leads a planted group: the next group - 1 rows are copies of it with 0, limit - 1, limit and limit + 1 columns
    changed to a letter the leader does not hold there (limit = max(int(max_diff_perc * columns), 1)), in that order, then repeating."""
    rng = np.random.default_rng(seed)
    text = np.empty((rows, columns), dtype=np.uint8)
    for c0 in range(0, rows, clade):
        ancestor = LETTERS[rng.integers(0, LETTERS.size, size=columns)]
        for i in range(c0, min(rows, c0 + clade)):
            row = ancestor.copy()
            redraw = rng.random(columns) < clade_rate
            row[redraw] = LETTERS[rng.integers(0, LETTERS.size, size=int(redraw.sum()))]
            text[i] = row
    limit = max(int(max_diff_perc * columns), 1)
    steps = [0, limit - 1, limit, limit + 1]
    for lead in range(0, rows, group_every):
        for k in range(1, group):
            if lead + k >= rows:
                break
            row = text[lead].copy()
            ndiff = min(steps[(k - 1) % 4], columns)
            cols = rng.choice(columns, size=ndiff, replace=False)
            row[cols] = np.where(row[cols] == ord("A"), ord("C"), ord("A")).astype(np.uint8)
            text[lead + k] = row
    return text


def ids_of(rows):
    return ["IMG_%d" % (2500000000 + k) for k in range(rows)]
