"""A plain Python/numpy statement of the near-identity call (include/checkm_hip.h, checkm_amd/csrc/nearid_dev.h): the counts of differing
columns, the limits, the bit rows and the band cuts of a budget.  Nothing here shares code with the library."""
import numpy as np

TILE = 64
MAX_ROWS, MAX_STRIDE, MAX_TEXT_BYTES = 1 << 17, 1 << 24, 1 << 34


def limit_of(row_len, max_diff_perc=0.08):
    """createSmallTree.py:66 and :72: near iff diffs == 0 or diffs < int(perc * len), which is diffs < max(int(perc * len), 1)."""
    return max(int(max_diff_perc * row_len), 1)


def diffs(text):
    """[n, n] int64: the columns at which rows i and j hold different bytes.  text: [n, row_len] uint8 (the rows without their padding)."""
    t = np.asarray(text, dtype=np.uint8)
    out = np.zeros((t.shape[0], t.shape[0]), dtype=np.int64)
    for i in range(t.shape[0]):
        out[i] = (t != t[i]).sum(axis=1)
    return out


def near_bits(text, limit):
    """[n, ceil(n / 64)] uint64: bit (j & 63) of word j // 64 of row i is set iff j > i and diffs(i, j) < limit[i]."""
    t = np.asarray(text, dtype=np.uint8)
    n = t.shape[0]
    d = diffs(t)
    words = (n + 63) // 64
    out = np.zeros((n, words), dtype=np.uint64)
    for i in range(n):
        for j in range(i + 1, n):
            if d[i, j] < int(limit[i]):
                out[i, j // 64] |= np.uint64(1 << (j % 64))
    return out


def bands(n_rows, row_stride, budget_bytes):
    """[(first row tile, one past the last)] of a call: the text and the limits stay resident, a row tile adds 64 bit rows; at least one
    row tile per band, then as many as the budget leaves room for."""
    words, tiles = (n_rows + 63) // 64, (n_rows + TILE - 1) // TILE
    fixed, per = n_rows * row_stride + n_rows * 4, TILE * words * 8
    n = max((budget_bytes - fixed) // per if budget_bytes > fixed else 0, 1)
    out, b0 = [], 0
    while b0 < tiles:
        b1 = min(tiles, b0 + n)
        out.append((b0, b1))
        b0 = b1
    return out


def refusal(text_present, n_rows, row_len, row_stride, limit):
    """None, or 'EINVAL' / 'ERANGE' as ckm_nearid_check answers, in the order of its tests."""
    if not text_present or limit is None:
        return 'EINVAL'
    if n_rows == 0 or row_len == 0 or row_stride < row_len or row_stride % 16:
        return 'EINVAL'
    if n_rows > MAX_ROWS or row_stride > MAX_STRIDE or n_rows * row_stride > MAX_TEXT_BYTES:
        return 'ERANGE'
    if any(int(x) == 0 for x in limit):
        return 'EINVAL'
    return None
