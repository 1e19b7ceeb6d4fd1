"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libselection_emu.so -- the layout, the generator, the draw, the packing and the round cuts
of the marker-set selection (checkm_amd/csrc/select_dev.h) compiled against a host executor.  select_check and select_run take the
arguments of their namesakes in checkm_amd._lib (ctx is ignored) and return the same.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libselection_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "selection_emu.cpp"), os.path.join(_CSRC, "select_dev.h"), os.path.join(_CSRC, "sim_dev.h"), os.path.join(_CSRC, "marker_sets.h"), os.path.join(_CSRC, "ckm_internal.h"), os.path.join(_HERE, "score_sets_emu.h"), os.path.join(_HERE, "..", "..", "include", "checkm_hip.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "selection_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        from checkm_amd._lib import SelectArgs
        L = C.CDLL(build())
        L.emu_select_check.argtypes = [C.POINTER(SelectArgs)]
        L.emu_select_run.argtypes = [C.POINTER(SelectArgs), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_philox.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_unit.argtypes = [C.c_uint32, C.c_uint32]
        L.emu_unit.restype = C.c_double
        _lib = L
    return _lib


def _refuse(rc):
    if rc:
        from checkm_amd import _lib as real
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)" % rc)


def philox(counter, key):
    c, k, w = np.asarray(counter, dtype=np.uint32), np.asarray(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    lib().emu_philox(c.ctypes.data, k.ctypes.data, w.ctypes.data)
    return [int(x) for x in w]


def unit(a, b):
    return lib().emu_unit(a, b)


def select_check(tables):
    a = tables.args()
    _refuse(lib().emu_select_check(C.byref(a)))


def select_run(ctx, tables, budget_bytes=0, with_rows=False):
    from checkm_amd import _lib as real
    a = tables.args()
    _refuse(lib().emu_select_check(C.byref(a)))
    truth, out, rows = real.select_arrays(tables, with_rows)
    truth[:], out[:] = np.nan, np.nan
    info = np.zeros(1, dtype=np.uint64)
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None
    _refuse(lib().emu_select_run(C.byref(a), int(budget_bytes) or (256 << 20), ptr(truth), ptr(out), ptr(rows) if with_rows else None, info.ctypes.data))
    return dict(truth=truth, out=out, rows=real.select_rows(tables, rows) if with_rows else None, nrounds=int(info[0]), ms_pack=0.0, ms_upload=0.0, ms_kernel=0.0,
                ms_download=0.0, ms_total=0.0)
