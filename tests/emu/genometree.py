"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libgenometree_emu.so -- the layout, the arithmetic and the batch cuts of the genome tree
(checkm_amd/csrc/gtree_dev.h) compiled against the header's host executor.  gtree_check and gtree_run take the arguments of their
namesakes in checkm_amd._lib (ctx is ignored) and return the same.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libgenometree_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "genometree_emu.cpp"), os.path.join(_CSRC, "gtree_dev.h"), os.path.join(_HERE, "..", "..", "include", "checkm_hip.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "genometree_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        from checkm_amd._lib import GtreeArgs, GtreeOut
        L = C.CDLL(build())
        L.emu_gtree_check.argtypes = [C.POINTER(GtreeArgs)]
        L.emu_gtree_run.argtypes = [C.POINTER(GtreeArgs), C.c_uint64, C.POINTER(GtreeOut), C.c_void_p]
        L.emu_gtree_log.argtypes = [C.c_double]
        L.emu_gtree_log.restype = C.c_double
        L.emu_gtree_dist.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_double]
        L.emu_gtree_dist.restype = C.c_double
        L.emu_gtree_arg.argtypes = [C.c_double, C.c_int]
        L.emu_gtree_arg.restype = C.c_double
        L.emu_gtree_logs.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def _refuse(rc):
    if rc:
        from checkm_amd import _lib as real
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)" % rc)


def log(x):
    return lib().emu_gtree_log(float(x))


def logs(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    lib().emu_gtree_logs(x.ctypes.data, x.size, y.ctypes.data)
    return y


def dist(compared, differ, model, max_dist):
    return lib().emu_gtree_dist(int(compared), int(differ), int(model), float(max_dist))


def arg(p, model):
    return lib().emu_gtree_arg(float(p), int(model))


def gtree_check(tables):
    a = tables.args()
    _refuse(lib().emu_gtree_check(C.byref(a)))


def gtree_run(ctx, tables, budget_bytes=0, counts=False, dist=False, merges=True):
    from checkm_amd import _lib as real
    info = np.zeros(2, dtype=np.uint64)

    def entry(a, budget, out, _info):
        rc = lib().emu_gtree_run(a, int(budget) or (2048 << 20), out, info.ctypes.data)
        return -7 if rc == 2 else -1 if rc else 0

    a = tables.args()
    _refuse(lib().emu_gtree_check(C.byref(a)))
    o = real._gtree_call(entry, tables, budget_bytes, counts, dist, merges)
    o["nrounds"], o["ntrees"] = int(info[0]), int(info[1])
    return o


def runner(tables, budget_bytes=0, **what):
    """What GenomeTree(runner=...) takes."""
    return gtree_run(None, tables, budget_bytes, **what)
