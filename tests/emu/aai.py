"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libaai_emu.so -- the per-chunk logic, the pair decode, the packing and the batches of
the all-pairs amino-acid identity (checkm_amd/csrc/aai_dev.h) compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libaai_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "aai_emu.cpp"), os.path.join(_CSRC, "aai_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", _LIB,
                               os.path.join(_HERE, "aai_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_aai_check.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p]
        L.emu_aai_run.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64] + [C.c_void_p] * 5
        L.emu_aai_decode.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
        L.emu_aai_decode.restype = None
        _lib = L
    return _lib


def decode(k, n):
    ij = np.zeros(2, dtype=np.uint32)
    lib().emu_aai_decode(int(k), int(n), ij.ctypes.data)
    return int(ij[0]), int(ij[1])


def aai_pairs(ctx, groups, budget_bytes=0):
    """checkm_amd._lib.aai_pairs on the host executor: same arguments (ctx is ignored), same dict."""
    from checkm_amd import _lib as real
    group_row_off, row_off, text = real._aai_args(groups)
    npairs = sum(len(g) * (len(g) - 1) // 2 for g in groups)
    pair_off = np.zeros(len(groups) + 1, dtype=np.uint64)
    mis, cmp_, val = np.full(max(1, npairs), -7, dtype=np.int32), np.full(max(1, npairs), -7, dtype=np.int32), np.full(max(1, npairs), np.nan)
    info = np.zeros(3, dtype=np.uint64)
    rc = lib().emu_aai_run(len(groups), group_row_off.ctypes.data, row_off.ctypes.data, text, int(budget_bytes) or (64 << 20), pair_off.ctypes.data, mis.ctypes.data,
                           cmp_.ctypes.data, val.ctypes.data, info.ctypes.data)
    if rc:
        raise real.CkmError(-7 if rc == 2 else -1, "the host executor refused the call")
    assert int(info[0]) == npairs
    return dict(npairs=npairs, nbatches=int(info[1]), bytes=int(info[2]), pair_off=pair_off, mismatches=mis[:npairs], compared=cmp_[:npairs], aai=val[:npairs],
                ms_pack=0.0, ms_upload=0.0, ms_kernel=0.0, ms_download=0.0, ms_total=0.0)
