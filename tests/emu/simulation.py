"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libsimulation_emu.so -- the layout, the arithmetic, the packing and the round cuts of the
marker-set simulation (checkm_amd/csrc/sim_dev.h) compiled against a host executor.  sim_check and sim_run take the arguments of their
namesakes in checkm_amd._lib (ctx is ignored) and return the same.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libsimulation_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "simulation_emu.cpp"), os.path.join(_CSRC, "sim_dev.h"), os.path.join(_CSRC, "marker_sets.h"), os.path.join(_CSRC, "ckm_internal.h"), os.path.join(_HERE, "score_sets_emu.h"), os.path.join(_HERE, "..", "..", "include", "checkm_hip.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "simulation_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        from checkm_amd._lib import SimArgs
        L = C.CDLL(build())
        L.emu_sim_check.argtypes = [C.POINTER(SimArgs)]
        L.emu_sim_run.argtypes = [C.POINTER(SimArgs), C.c_uint64, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _refuse(rc):
    if rc:
        from checkm_amd import _lib as real
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)" % rc)


def sim_check(tables):
    a = tables.args()
    _refuse(lib().emu_sim_check(C.byref(a)))


def sim_run(ctx, tables, budget_bytes=0):
    out = np.full((tables.nreplicates, tables.nsets, 4), np.nan, dtype=np.float64)
    info, a = np.zeros(1, dtype=np.uint64), tables.args()
    _refuse(lib().emu_sim_run(C.byref(a), int(budget_bytes) or (256 << 20), out.ctypes.data if out.size else None, info.ctypes.data))
    return dict(out=out, nrounds=int(info[0]), ms_pack=0.0, ms_upload=0.0, ms_kernel=0.0, ms_download=0.0, ms_total=0.0)
