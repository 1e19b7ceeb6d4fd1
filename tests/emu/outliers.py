"""TEST INFRASTRUCTURE: ctypes face of tests/emu/liboutliers_emu.so -- the arithmetic of the outlier pass
(checkm_amd/csrc/outlier_dev.h) compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "liboutliers_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "outliers_emu.cpp"), os.path.join(_CSRC, "outlier_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", _LIB, os.path.join(_HERE, "outliers_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_td.argtypes = [C.c_void_p, C.c_void_p]
        L.emu_td.restype = C.c_double
        L.emu_nearest_key.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.emu_outliers.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 10 + [C.c_uint32] + [C.c_void_p] * 10
        _lib = L
    return _lib


def td(row, binsig):
    row, binsig = np.ascontiguousarray(row, dtype=np.float64), np.ascontiguousarray(binsig, dtype=np.float64)
    assert row.shape == binsig.shape == (136,)
    return lib().emu_td(row.ctypes.data, binsig.ctypes.data)


def nearest_key(keys, length):
    k = np.ascontiguousarray(keys, dtype=np.float64)
    return int(lib().emu_nearest_key(k.ctypes.data, len(k), float(length)))


def outliers(bin_first, count, sig, coding, tab_off, key, lo, hi, bin_gc_tab, bin_cd_tab, td_tab):
    """Same result layout as checkm_amd._lib.outliers (without the timings)."""
    bin_first = np.ascontiguousarray(bin_first, dtype=np.uint32)
    nbins, nseq = len(bin_first) - 1, int(bin_first[-1])
    count = np.ascontiguousarray(count, dtype=np.uint64)
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    coding = np.ascontiguousarray(coding, dtype=np.int64)
    assert count.shape == (nseq, 8) and sig.shape == (nseq, 136) and coding.shape == (nseq,)
    tab_off = np.ascontiguousarray(tab_off, dtype=np.uint32)
    key, lo, hi = (np.ascontiguousarray(x, dtype=np.float64) for x in (key, lo, hi))
    gct, cdt = (np.ascontiguousarray(x, dtype=np.uint32) for x in (bin_gc_tab, bin_cd_tab))
    out = {f: np.zeros(nseq) for f in ("gc", "delta_gc", "cd", "delta_cd", "td", "weight")}
    out["flags"] = np.zeros(nseq, dtype=np.uint8)
    out["mean_gc"], out["mean_cd"], out["bin_sig"] = np.zeros(nbins), np.zeros(nbins), np.zeros((nbins, 136))
    rc = lib().emu_outliers(nseq, nbins, bin_first.ctypes.data, count.ctypes.data, coding.ctypes.data, sig.ctypes.data, tab_off.ctypes.data,
                            key.ctypes.data, lo.ctypes.data, hi.ctypes.data, gct.ctypes.data, cdt.ctypes.data, int(td_tab),
                            *[out[f].ctypes.data for f in ("gc", "delta_gc", "cd", "delta_cd", "td", "weight", "flags", "mean_gc", "mean_cd", "bin_sig")])
    if rc == -1:
        raise ZeroDivisionError("float division by zero")
    assert rc == 0, rc
    return out
