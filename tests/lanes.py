"""The build helper of the lane emulation (tests/test_*_lanes_cpu.py, DESIGN.md "Lane emulation harness"): a translation unit of
tests/lane_emulation/ -- on_host.h, a csrc/*.hip file and perhaps a main -- compiled as host C++ over the stand-in runtime of
tests/lane_emulation/hip/hip_runtime.h, as a shared object for ctypes or as a sanitized stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "lane_emulation")
# -O1 and no contraction: the differences to the references that the tests' docstrings state were measured with them
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-Wno-psabi",
         "-I", HERE, "-I", os.path.join(ROOT, "pixel-perfect-sfm_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
_loaded = {}


def _clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cand = [os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
            shutil.which("clang++")]
    return next((c for c in cand if c and os.path.exists(c)), None)


def compile(source, out, *flags):
    """tests/lane_emulation/<source> to `out`."""
    cxx = _clang()       # the device headers use clang's vector types: the compiler that hipcc drives, as a plain host compiler
    assert cxx, "no clang++ next to hipcc"
    subprocess.check_call([cxx, *FLAGS, *flags, os.path.join(HERE, source), "-o", str(out)])


def load(tmp_path_factory, source):
    """(lib, ctx) of tests/lane_emulation/<source> as a shared object, built once per session."""
    if source not in _loaded:
        out = tmp_path_factory.mktemp("lanes") / ("lib%s.so" % os.path.splitext(source)[0])
        compile(source, out, "-shared")
        lib = C.CDLL(str(out))
        lib.emu_ctx.restype = C.c_void_p
        lib.emu_last_error.restype = C.c_char_p
        _loaded[source] = lib, C.c_void_p(lib.emu_ctx())
    return _loaded[source]


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(lib, rc):
    if rc:
        raise ValueError("%d: %s" % (rc, lib.emu_last_error().decode()))


def sanitized(tmp_path, source, macro, *args):
    """One run of tests/lane_emulation/<source> with its own main (-D<macro>) under AddressSanitizer and UndefinedBehaviorSanitizer,
    as a stand-alone host program (built once per tmp_path); returns what it printed."""
    exe = tmp_path / macro.lower()
    if not exe.exists():       # line tables are what a sanitizer's report needs; full -g takes a minute longer on the matching translation unit
        compile(source, exe, "-D" + macro, "-gline-tables-only", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    res = subprocess.run([str(exe), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    return res.stdout
