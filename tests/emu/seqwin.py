"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libseqwin_emu.so -- the piece logic of the sequence-window pass
(checkm_amd/csrc/seqwin_dev.h) and the distance of outlier_dev.h compiled against a host executor.  Never imported by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libseqwin_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "seqwin_emu.cpp")] + [os.path.join(_CSRC, h) for h in ("seqwin_dev.h", "nucstats_dev.h", "outlier_dev.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", _LIB, os.path.join(_HERE, "seqwin_emu.cpp")])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_seq_windows_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64] + \
                                         [C.c_void_p] * 6
        _lib = L
    return _lib


def seq_windows(ctx, seqs, window_size, bin_sig=None, want_tetra=False, piece_bytes=0, budget_bytes=0):
    """checkm_amd._lib.seq_windows on the host executor: same arguments (ctx is ignored, seqs is a checkm_amd._lib.NucSeqs), same dict."""
    from checkm_amd import _lib as product
    first = product.seq_windows_layout(seqs, window_size)
    nwin, nseq = int(first[-1]), seqs.nseq
    base = np.zeros((max(1, nwin), 4), dtype=np.uint32)
    per_seq = np.zeros((max(1, nseq), 4), dtype=np.uint64)
    skipped = np.zeros(max(1, nseq), dtype=np.uint8)
    info = np.zeros(4, dtype=np.uint64)
    td = tetra = sig = None
    if bin_sig is not None:
        sig = np.ascontiguousarray(bin_sig, dtype=np.float64)
        assert sig.shape == (seqs.nfiles, 136)
        td = np.zeros(max(1, nwin), dtype=np.float64)
    if want_tetra:
        tetra = np.zeros((max(1, nwin), 136), dtype=np.uint32)
    off, nbytes, ff = (np.ascontiguousarray(x) for x in (seqs.seq_off, seqs.seq_bytes, seqs.file_first))
    rc = lib().emu_seq_windows_run(seqs._view.text, off.ctypes.data, nbytes.ctypes.data, ff.ctypes.data, nseq, seqs.nfiles, int(window_size),
                                   1 if (sig is not None or want_tetra) else 0, sig.ctypes.data if sig is not None else None, int(piece_bytes) or 4096,
                                   int(budget_bytes) or (1024 << 20), base.ctypes.data, per_seq.ctypes.data, td.ctypes.data if td is not None else None,
                                   tetra.ctypes.data if tetra is not None else None, skipped.ctypes.data, info.ctypes.data)
    if rc:
        raise product.CkmError(rc, "host executor refused the call")
    return dict(first=first, base=base[:nwin], seq=per_seq[:nseq], td=None if td is None else td[:nwin], tetra=None if tetra is None else tetra[:nwin],
                skipped=skipped[:nseq].astype(bool), windows=int(info[0]), pieces=int(info[1]), batches=int(info[2]), bytes=0, skipped_seqs=int(info[3]),
                ms_upload=0.0, ms_count=0.0, ms_td=0.0, ms_download=0.0, ms_total=0.0)
