"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libmarkerset_emu.so -- the arithmetic, the rounds, the tile lists and the output batches of
MarkerSetBuilder (checkm_amd/csrc/markerset_dev.h) compiled against a host executor.  MsetTable, mset_check, mset_markers and
mset_colocated take the arguments of their namesakes in checkm_amd._lib (ctx is ignored) and return the same dicts.  Never imported by
checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libmarkerset_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "markerset_emu.cpp"), os.path.join(_CSRC, "markerset_dev.h"), os.path.join(_CSRC, "pairs_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "markerset_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        table = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_mset_check.argtypes = table + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
        L.emu_mset_markers.argtypes = table + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_mset_colocated.argtypes = table + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint64, C.c_void_p]
        L.emu_mset_fetch.argtypes = [C.c_void_p] * 4
        L.emu_mset_fetch.restype = None
        _lib = L
    return _lib


def _real():
    from checkm_amd import _lib as real
    return real


def _refuse(rc):
    if rc:
        raise _real().CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)" % rc)


_MS = ("ms_upload", "ms_markers", "ms_pack", "ms_count", "ms_scan", "ms_fill", "ms_download", "ms_total")


def mset_check(count_class, pos_off, pos, genome_lists=None, marker_lists=None, dist_threshold=5000):
    real = _real()
    G, Cn, cls, off, p = real._mset_table_args(count_class, pos_off, pos)
    goff, g = real._mset_lists(genome_lists) if genome_lists is not None else (None, None)
    moff, m = real._mset_lists(marker_lists) if marker_lists is not None else (None, None)
    _refuse(lib().emu_mset_check(G, Cn, real._ptr(cls), off.ctypes.data, real._ptr(p), len(genome_lists) if genome_lists is not None else 0,
                                 goff.ctypes.data if goff is not None else None, real._ptr(g) if g is not None else None,
                                 moff.ctypes.data if moff is not None else None, real._ptr(m) if m is not None else None, float(dist_threshold)))


class MsetTable(object):
    def __init__(self, ctx, count_class, pos_off, pos):
        real = _real()
        self.ngenomes, self.nfamilies, self.cls, self.off, self.pos = real._mset_table_args(count_class, pos_off, pos)
        _refuse(lib().emu_mset_check(*(self.args() + (0, None, None, None, None, 0.0))))
        self.ms_upload = 0.0

    def args(self):
        real = _real()
        return (self.ngenomes, self.nfamilies, real._ptr(self.cls), self.off.ctypes.data, real._ptr(self.pos))

    def close(self):
        pass


def mset_markers(ctx, table, genome_lists, ubiquity_thresholds, single_copy_thresholds, want_counts=False, budget_bytes=0):
    real = _real()
    goff, g = real._mset_lists(genome_lists)
    tu = np.ascontiguousarray(ubiquity_thresholds, dtype=np.float64).reshape(-1)
    ts = np.ascontiguousarray(single_copy_thresholds, dtype=np.float64).reshape(-1)
    nq = len(genome_lists)
    assert tu.shape[0] == nq and ts.shape[0] == nq
    flag = np.full((nq, table.nfamilies), 0xEE, dtype=np.uint8)
    counts = np.full((nq, table.nfamilies, 3), 0xEEEEEEEE, dtype=np.uint32) if want_counts else None
    _refuse(lib().emu_mset_markers(*(table.args() + (nq, goff.ctypes.data, real._ptr(g), real._ptr(tu), real._ptr(ts), real._ptr(flag),
                                                     real._ptr(counts) if want_counts else None))))
    return dict(dict.fromkeys(_MS, 0.0), nbatches=1, flag=flag, counts=counts)


def mset_colocated(ctx, table, genome_lists, marker_lists, dist_threshold=5000, genome_threshold=0.95, budget_bytes=0):
    real = _real()
    assert len(genome_lists) == len(marker_lists)
    goff, g = real._mset_lists(genome_lists)
    moff, m = real._mset_lists(marker_lists)
    nq = len(genome_lists)
    info = np.zeros(4, dtype=np.uint64)
    _refuse(lib().emu_mset_colocated(*(table.args() + (nq, goff.ctypes.data, real._ptr(g), moff.ctypes.data, real._ptr(m), float(dist_threshold), float(genome_threshold),
                                                       int(budget_bytes) or (256 << 20), info.ctypes.data))))
    k = int(info[0])
    pair_off = np.zeros(nq + 1, dtype=np.uint64)
    i, j, count = (np.zeros(k, dtype=np.uint32) for _ in range(3))
    lib().emu_mset_fetch(pair_off.ctypes.data, real._ptr(i), real._ptr(j), real._ptr(count))
    return dict(dict.fromkeys(_MS, 0.0), npairs=k, nbatches=int(info[1]), nrounds=int(info[2]), tests=int(info[3]), pair_off=pair_off, i=i, j=j, count=count)
