"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libplacement_emu.so -- the layout, the arithmetic, the level schedule and the chunk cuts of
the phylogenetic placement (checkm_amd/csrc/place_dev.h) compiled against its host executor.  place_check and place_run take the
arguments of their namesakes in checkm_amd._lib (ctx is ignored) and return the same.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libplacement_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "placement_emu.cpp"), os.path.join(_CSRC, "place_dev.h"), os.path.join(_HERE, "..", "..", "include", "checkm_hip.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "placement_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        from checkm_amd._lib import PlaceArgs, PlaceOut
        L = C.CDLL(build())
        L.emu_place_check.argtypes = [C.POINTER(PlaceArgs)]
        L.emu_place_run.argtypes = [C.POINTER(PlaceArgs), C.c_uint64, C.POINTER(PlaceOut), C.c_void_p]
        L.emu_place_levels.argtypes = [C.POINTER(PlaceArgs)] + [C.c_void_p] * 5
        _lib = L
    return _lib


def _refuse(rc):
    if rc:
        from checkm_amd import _lib as real
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call (%d)" % rc)


def place_check(tables):
    a = tables.args()
    _refuse(lib().emu_place_check(C.byref(a)))


def place_run(ctx, tables, budget_bytes=0):
    o, po = tables.outputs()
    info, a = np.zeros(2, dtype=np.uint64), tables.args()
    _refuse(lib().emu_place_run(C.byref(a), int(budget_bytes) or (2048 << 20), C.byref(po), info.ctypes.data))
    o.update(nchunks=int(info[0]), chunk_sites=int(info[1]), ms_total=0.0)
    return o


def place_levels(tables):
    """The level schedule: (upward levels as lists of nodes, downward levels as lists of edges)."""
    n = tables.nnodes
    up_off, up, down_off, down, nd = (np.zeros(k, dtype=np.uint32) for k in (n + 2, n, n + 1, n, 1))
    a = tables.args()
    nu = lib().emu_place_levels(C.byref(a), up_off.ctypes.data, up.ctypes.data, down_off.ctypes.data, down.ctypes.data, nd.ctypes.data)
    if nu < 0:
        _refuse(1)
    return ([up[up_off[k]:up_off[k + 1]].tolist() for k in range(nu)], [down[down_off[k]:down_off[k + 1]].tolist() for k in range(int(nd[0]))])
