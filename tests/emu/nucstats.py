"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libnucstats_emu.so -- the tile logic of the nucleotide statistics pass
(checkm_amd/csrc/nucstats_dev.h) compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libnucstats_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "nucstats_emu.cpp"), os.path.join(_CSRC, "nucstats_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", _LIB, os.path.join(_HERE, "nucstats_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_nucstats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def nucstats(seqs, tile_bytes):
    """Same result layout as checkm_amd._lib.nucstats (count, piece_off, piece_len, tetra) for a list of byte strings."""
    off, pos = [], 0
    for s in seqs:
        off.append(pos)
        pos += (len(s) + 15) & ~15
    text = np.zeros(pos + 64, dtype=np.uint8)
    for o, s in zip(off, seqs):
        text[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    n = len(seqs)
    seq_off = np.asarray(off, dtype=np.uint64)
    seq_bytes = np.asarray([len(s) for s in seqs], dtype=np.uint64)
    count = np.zeros((max(1, n), 8), dtype=np.uint64)
    tetra = np.zeros((max(1, n), 136), dtype=np.uint32)
    piece_off = np.zeros(n + 1, dtype=np.uint64)
    cap = pos + n + 1
    piece_len = np.zeros(cap, dtype=np.uint64)
    rc = lib().emu_nucstats(text.ctypes.data, seq_off.ctypes.data, seq_bytes.ctypes.data, n, int(tile_bytes), count.ctypes.data, tetra.ctypes.data,
                            piece_off.ctypes.data, piece_len.ctypes.data, cap)
    assert rc == 0, rc
    return dict(count=count[:n], piece_off=piece_off, piece_len=piece_len[:int(piece_off[-1])], tetra=tetra[:n])
