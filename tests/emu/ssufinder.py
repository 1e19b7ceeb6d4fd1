"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libssufinder_emu.so -- the score system, the check, the tile cuts, the compaction order
and the hit rule of the nucleotide model scan (checkm_amd/csrc/nhmm_dev.h) compiled against its host executor.  nhmm_check and nhmm_run
take the arguments of their namesakes in checkm_amd._lib (ctx is ignored; the sequences are a _lib.NucSeqs, read by the library's host
code) and return the same.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libssufinder_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "ssufinder_emu.cpp"), os.path.join(_CSRC, "nhmm_dev.h"), os.path.join(_HERE, "..", "..", "include", "checkm_hip.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", _LIB,
                               os.path.join(_HERE, "ssufinder_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        from checkm_amd._lib import NhmmArgs, NhmmColumns
        L = C.CDLL(build())
        L.emu_nhmm_check.argtypes = [C.POINTER(NhmmArgs)]
        L.emu_nhmm_run.argtypes = [C.POINTER(NhmmArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]
        L.emu_nhmm_columns.argtypes = [C.c_void_p, C.POINTER(NhmmColumns)]
        L.emu_nhmm_columns.restype = None
        L.emu_nhmm_free.argtypes = [C.c_void_p]
        L.emu_nhmm_free.restype = None
        L.emu_nhmm_tbm.argtypes = [C.c_uint32]
        L.emu_nhmm_hits.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32] + [C.c_void_p] * 6
        _lib = L
    return _lib


def _refuse(rc, what=""):
    if rc:
        from checkm_amd import _lib as real
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)%s" % (rc, what))


def tbm(M):
    return int(lib().emu_nhmm_tbm(int(M)))


def nhmm_check(tables):
    a = tables.args()
    _refuse(lib().emu_nhmm_check(C.byref(a)))


def nhmm_run(ctx, tables, seqs, budget_bytes=0):
    from checkm_amd import _lib as real
    h, info, a = C.c_void_p(), np.zeros(5, dtype=np.int64), tables.args()
    off, nbytes = np.ascontiguousarray(seqs.seq_off, dtype=np.uint64), np.ascontiguousarray(seqs.seq_bytes, dtype=np.uint64)
    rc = lib().emu_nhmm_run(C.byref(a), seqs._view.text, off.ctypes.data, nbytes.ctypes.data, seqs.nseq, int(budget_bytes) or (256 << 20), C.byref(h), info.ctypes.data)
    _refuse(rc, ": sequence %s" % seqs.ids()[int(info[4])] if info[4] >= 0 else "")
    try:
        c = real.NhmmColumns()
        lib().emu_nhmm_columns(h, C.byref(c))
        ns = types.SimpleNamespace(tiles=info[0], launches=info[1], cells=info[2], batches=info[3], **{f: 0.0 for f in real._NHMM_MS})
        return real.nhmm_columns(c, ns)
    finally:
        lib().emu_nhmm_free(h)


def hits_of(rows, L, strand=0):
    """The hit rule on reported rows [(start, row, score)] of one strand of a sequence of L bases: [(from, to, score)] as accepted."""
    n = len(rows)
    a = [np.ascontiguousarray([r[k] for r in rows], dtype=np.int32 if k == 2 else np.uint32) for k in range(3)]
    o = [np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.int32)]
    k = lib().emu_nhmm_hits(n, int(L), int(strand), *[x.ctypes.data for x in a + o])
    return [(int(o[0][i]), int(o[1][i]), int(o[2][i])) for i in range(k)]
