"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libunbinned_emu.so -- the per-word logic and the tile geometry of the selective base
count of `checkm unbinned` (checkm_amd/csrc/unbinned_dev.h) compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libunbinned_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "unbinned_emu.cpp"), os.path.join(_CSRC, "unbinned_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", _LIB,
                               os.path.join(_HERE, "unbinned_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_unbinned_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def count_raw(text, seq_off, seq_bytes, keep, tile_bytes, budget_bytes):
    """The host executor over a text buffer laid out as the reader lays it out (bytes, a numpy uint8 array or an address): (counts
    [nseq, 5] uint64, info [4] uint64 = kept, tiles, batches, bytes)."""
    off, nbytes, keep = (np.ascontiguousarray(seq_off, dtype=np.uint64), np.ascontiguousarray(seq_bytes, dtype=np.uint64), np.ascontiguousarray(keep, dtype=np.uint8))
    n = len(off)
    counts = np.zeros((max(1, n), 5), dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    addr = text.ctypes.data if isinstance(text, np.ndarray) else text
    rc = lib().emu_unbinned_count(addr, off.ctypes.data, nbytes.ctypes.data, n, keep.ctypes.data if n else counts.ctypes.data, int(tile_bytes), int(budget_bytes),
                                  counts.ctypes.data, info.ctypes.data)
    if rc:
        raise ValueError("host executor refused the call")
    return counts[:n], info


def unbinned_count(ctx, seqs, keep, tile_bytes=0, budget_bytes=0):
    """checkm_amd._lib.unbinned_count on the host executor: same arguments (ctx is ignored, seqs is a checkm_amd._lib.NucSeqs), same dict."""
    counts, info = count_raw(seqs._view.text, seqs.seq_off, seqs.seq_bytes, keep, int(tile_bytes) or 4096, int(budget_bytes) or (1024 << 20))
    return dict(counts=counts, kept=int(info[0]), tiles=int(info[1]), batches=int(info[2]), bytes=int(info[3]), ms_stage=0.0, ms_upload=0.0, ms_count=0.0, ms_sum=0.0,
                ms_download=0.0, ms_total=0.0)
