"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libmerge_emu.so -- the all-pairs comparison of `checkm merge`
(checkm_amd/csrc/merge_dev.h, merge_host.h) compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libmerge_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None

COLUMNS = ("comp_i", "cont_i", "comp_j", "cont_j", "delta_comp", "delta_cont", "delta", "comp_merged", "cont_merged")


def build(force=False):
    srcs = [os.path.join(_HERE, "merge_emu.cpp"), os.path.join(_CSRC, "merge_dev.h"), os.path.join(_CSRC, "merge_host.h"), os.path.join(_CSRC, "pairs_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", _LIB, os.path.join(_HERE, "merge_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_merge.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_uint64, C.POINTER(C.c_uint64)]
        L.emu_merge.restype = C.c_int64
        L.emu_merge_lines.argtypes = [C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64]
        L.emu_merge_lines.restype = C.c_uint64
        L.emu_merge_check.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
        _lib = L
    return _lib


def _args(bits, hit_sum, n_markers, thr):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    return bits, np.ascontiguousarray(hit_sum, dtype=np.int64), np.ascontiguousarray(n_markers, dtype=np.int32), np.ascontiguousarray(thr, dtype=np.float64)


def merge_pairs(bits, hit_sum, n_markers, ngenes, thr, cap_pairs=0, pass_rows=0):
    """Same result layout as checkm_amd._lib.merge_pairs (without the timings)."""
    bits, s, n, t = _args(bits, hit_sum, n_markers, thr)
    nb = bits.shape[0]
    max_out = max(1, nb * (nb - 1) // 2)
    oi, oj = np.zeros(max_out, dtype=np.uint32), np.zeros(max_out, dtype=np.uint32)
    cols = np.zeros((9, max_out))
    nbatches = C.c_uint64(0)
    k = lib().emu_merge(nb, int(ngenes), bits.ctypes.data, s.ctypes.data, n.ctypes.data, t.ctypes.data, int(cap_pairs), int(pass_rows),
                        oi.ctypes.data, oj.ctypes.data, cols.ctypes.data, max_out, C.byref(nbatches))
    if k == -1:
        raise ValueError("refused arguments")
    assert k >= 0, k
    out = dict(npairs=int(k), compared=nb * (nb - 1) // 2, nbatches=int(nbatches.value), i=oi[:k].copy(), j=oj[:k].copy())
    for q, f in enumerate(COLUMNS):
        out[f] = cols[q, :k].copy()
    return out


def lines(ids, res):
    """The bytes ckm_merge_run appends to merger.tsv for the pairs of a merge_pairs() result."""
    k = res["npairs"]
    cols = np.ascontiguousarray(np.stack([res[f] for f in COLUMNS])) if k else np.zeros((9, 1))
    arr = (C.c_char_p * max(1, len(ids)))(*[b if isinstance(b, bytes) else b.encode() for b in ids])
    i, j = np.ascontiguousarray(res["i"], dtype=np.uint32), np.ascontiguousarray(res["j"], dtype=np.uint32)
    cap = 64 + k * (2 * max([len(b) for b in arr[:len(ids)]] + [1]) + 9 * 12 + 16)
    buf = C.create_string_buffer(cap)
    n = lib().emu_merge_lines(arr, i.ctypes.data, j.ctypes.data, cols.ctypes.data, cols.shape[1], k, buf, cap)
    assert n <= cap, (n, cap)
    return buf.raw[:n]


def check(bits, hit_sum, n_markers, ngenes, thr):
    """'' when the library would compute these arguments, else its reason."""
    bits, s, n, t = _args(bits, hit_sum, n_markers, thr)
    why = C.create_string_buffer(256)
    lib().emu_merge_check(bits.shape[0], int(ngenes), bits.ctypes.data, s.ctypes.data, n.ctypes.data, t.ctypes.data, why, 256)
    return why.value.decode()
