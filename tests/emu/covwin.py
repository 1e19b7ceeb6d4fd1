"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libcovwin_emu.so -- the device pass of CoverageWindows
(checkm_amd/csrc/covwin_dev.h), its scan and the library's BAM reader (bam_host.cpp) compiled against a host executor.  Never imported
by checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu.coverage import RecordError, Refused          # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libcovwin_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, "covwin_emu.cpp")] + [os.path.join(_CSRC, f) for f in ("covwin_dev.h", "coverage_dev.h", "bam_host.h", "bam_host.cpp", "host_pool.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-I", _CSRC, "-o", _LIB, os.path.join(_HERE, "covwin_emu.cpp"), os.path.join(_CSRC, "bam_host.cpp"), "-lz"])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_covwin.argtypes = [C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_int64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                 C.c_void_p, C.c_char_p, C.c_uint32]
        _lib = L
    return _lib


def windows(path, all_reads, min_align_per, max_edit_dist_per, window, budget=0, threads=3, cap_refs=4096, cap_slots=1 << 21):
    """([n_ref, 9] int64, first slots [n_ref + 1], depth sums [slots], info dict) as ckm_coverage_windows_run computes them; Refused /
    RecordError where the library refuses."""
    out, first, sums, info = np.zeros((cap_refs, 9), dtype=np.int64), np.zeros(cap_refs + 1, dtype=np.int64), np.zeros(cap_slots, dtype=np.int64), np.zeros(5, dtype=np.uint64)
    why = C.create_string_buffer(1024)
    rc = lib().emu_covwin(os.fsencode(path), float(min_align_per), float(max_edit_dist_per), 1 if all_reads else 0, max(-1, min(int(window), 1 << 62)), int(budget), threads,
                          out.ctypes.data, cap_refs, first.ctypes.data, sums.ctypes.data, cap_slots, info.ctypes.data, why, 1024)
    if rc == -2:
        raise RecordError(int(info[3]), why.value.decode(errors="replace"))
    if rc != 0:
        raise Refused(why.value.decode(errors="replace"))
    return out, first, sums[:int(info[4])].copy(), dict(records=int(info[0]), batches=int(info[1]), atomics=int(info[2]), slots=int(info[4]))
