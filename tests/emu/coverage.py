"""TEST INFRASTRUCTURE: ctypes face of tests/emu/libcoverage_emu.so -- the device pass of `checkm coverage`
(checkm_amd/csrc/coverage_dev.h) and the library's BAM reader (bam_host.cpp) compiled against a host executor.  Never imported by
checkm_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libcoverage_emu.so")
_CSRC = os.path.join(_HERE, "..", "..", "checkm_amd", "csrc")
_lib = None


class Refused(ValueError):
    pass


class RecordError(ValueError):
    def __init__(self, slot, read):
        ValueError.__init__(self, "record %d, reason %d, read %r" % (slot >> 3, slot & 7, read))
        self.record, self.reason, self.read = slot >> 3, slot & 7, read


def build(force=False):
    srcs = [os.path.join(_HERE, "coverage_emu.cpp")] + [os.path.join(_CSRC, f) for f in ("coverage_dev.h", "bam_host.h", "bam_host.cpp", "host_pool.h")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-I", _CSRC, "-o", _LIB, os.path.join(_HERE, "coverage_emu.cpp"), os.path.join(_CSRC, "bam_host.cpp"), "-lz"])
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_coverage.argtypes = [C.c_char_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint32]
        L.emu_bam_scan.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint32]
        _lib = L
    return _lib


def scan(path, budget=0, threads=3, cap_refs=4096, cap_off=1 << 20):
    """(names, lengths, record offsets in the inflated stream, batches, header bytes) by the library's reader."""
    names = C.create_string_buffer(1 << 20)
    lengths, off, info = np.zeros(cap_refs, dtype=np.int64), np.zeros(cap_off, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    why = C.create_string_buffer(1024)
    rc = lib().emu_bam_scan(os.fsencode(path), int(budget), threads, names, len(names), lengths.ctypes.data, cap_refs, off.ctypes.data, cap_off, info.ctypes.data, why, 1024)
    if rc != 0:
        raise Refused(why.value.decode(errors="replace"))
    n = int(info[0])
    assert n <= cap_refs and int(info[1]) <= cap_off
    return names.value.decode("utf-8").split("\n")[:n], lengths[:n].tolist(), off[:int(info[1])].copy(), int(info[2]), int(info[3])


def counters(path, all_reads, min_align_per, max_edit_dist_per, min_qc, budget=0, threads=3, cap_refs=4096):
    """([n_ref, 9] int64, info dict) as ckm_coverage_run computes them; Refused / RecordError where the library refuses."""
    out, info = np.zeros((cap_refs, 9), dtype=np.int64), np.zeros(4, dtype=np.uint64)
    why = C.create_string_buffer(1024)
    rc = lib().emu_coverage(os.fsencode(path), float(min_align_per), float(max_edit_dist_per), float(min_qc), 1 if all_reads else 0, int(budget), threads,
                            out.ctypes.data, cap_refs, info.ctypes.data, why, 1024)
    if rc == -2:
        raise RecordError(int(info[3]), why.value.decode(errors="replace"))
    if rc != 0:
        raise Refused(why.value.decode(errors="replace"))
    return out, dict(records=int(info[0]), batches=int(info[1]), atomics=int(info[2]))
