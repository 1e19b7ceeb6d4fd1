"""TEST INFRASTRUCTURE: ctypes face of tests/emu/librefdist_emu.so -- the geometry of the reference-distribution pass
(checkm_amd/csrc/refdist_dev.h), the lane step of seqwin_dev.h and the distance of outlier_dev.h compiled against a host executor.
Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "librefdist_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "refdist_emu.cpp")] + [os.path.join(_CSRC, h) for h in ("refdist_dev.h", "seqwin_dev.h", "nucstats_dev.h", "outlier_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", _LIB, os.path.join(_HERE, "refdist_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_refdist_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + \
                                     [C.c_void_p] * 4
        _lib = L
    return _lib


def refdist(ctx, seqs, stat, sep_len, starts, sizes, block=0, budget_bytes=0):
    """checkm_amd._lib.refdist on the host executor: same arguments (ctx is ignored, seqs is a checkm_amd._lib.NucSeqs), same dict."""
    from checkm_amd import _lib as product
    a, w = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(sizes, dtype=np.int64)
    n, code = len(a), product.REFDIST_STATS[stat]
    counts = np.zeros((max(1, n), 2), dtype=np.uint32) if code != 2 else None
    td = np.zeros(max(1, n), dtype=np.float64) if code == 2 else None
    totals = np.zeros(138, dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    off, nbytes = np.ascontiguousarray(seqs.seq_off), np.ascontiguousarray(seqs.seq_bytes)
    rc = lib().emu_refdist_run(seqs._view.text, off.ctypes.data, nbytes.ctypes.data, seqs.nseq, code, int(sep_len), int(block), a.ctypes.data, w.ctypes.data, n,
                               int(budget_bytes) or (1024 << 20), counts.ctypes.data if counts is not None else None, td.ctypes.data if td is not None else None,
                               totals.ctypes.data, info.ctypes.data)
    if rc:
        raise product.CkmError(rc, "host executor refused the call")
    return dict(counts=None if counts is None else counts[:n], td=None if td is None else td[:n], totals=totals, windows=int(info[0]), blocks=int(info[1]),
                batches=int(info[2]), bytes=int(info[3]), ms_scaffold=0.0, ms_upload=0.0, ms_blocks=0.0, ms_scan=0.0, ms_windows=0.0, ms_download=0.0, ms_total=0.0)
