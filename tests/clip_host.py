"""What the host tests of the clip features (tests/test_clip_*_host.py) share: the build of a kernel's emulator
(tests/host_emul/<stem>_emul.cpp), the run of a sanitizer program (tools/sanitize/<stem>.c) and the ctypes mirrors of the
descriptors every clip kernel reads.  A helper module: no test, no fixture."""
import ctypes as C
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class MelDesc(C.Structure):                        # include/pdmp3_hip.h pdmp3_mel_desc
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("src_chan_stride", C.c_uint64), ("dst_chan_stride", C.c_uint64),
                ("lead", C.c_uint32), ("pad_", C.c_uint32)]


class FbankDesc(C.Structure):                      # include/pdmp3_hip.h pdmp3_fbank_desc
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("src_chan_stride", C.c_uint64), ("dst_chan_stride", C.c_uint64),
                ("valid", C.c_uint32), ("pad_", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def build_emul(stem, extra=()):
    """tests/host_emul/<stem>_emul.cpp compiled into tests/host_emul/lib<stem>_emul.so (extra: further g++ arguments) and
    loaded -> the CDLL, once per (stem, extra); argtypes, restypes and size assertions are the caller's"""
    d = os.path.join(ROOT, "tests", "host_emul")
    so = os.path.join(d, "lib%s_emul.so" % stem)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(d, "%s_emul.cpp" % stem)] + list(extra))
    return C.CDLL(so)


def run_sanitizer_program(tmp_path, stem, host_sources):
    """tools/sanitize/<stem>.c with pdmp3_amd/host/<host_sources> as a stand-alone program under AddressSanitizer and UBSan on
    the CPU: built into tmp_path, run, and held to exit status 0 and its closing "<stem>: ok" line"""
    exe = str(tmp_path / (stem + "_sanitize"))
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "pdmp3_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "sanitize", stem + ".c")] +
                          [os.path.join(ROOT, "pdmp3_amd", "host", c) for c in host_sources] + ["-lm", "-w"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout.decode()
    assert stem.encode() + b": ok" in r.stdout
