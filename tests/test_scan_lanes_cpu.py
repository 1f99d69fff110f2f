"""The integer prefix sums of csrc/pxr_scan.h, run lane by lane on the CPU: the header is compiled as host C++ over the stand-in
runtime of tests/lane_emulation and held to numpy.cumsum in the output type, exactly -- the wave scan and its carry through LDS at
one, four and sixteen wavefronts, the reuse of s_part by a second call, wrap-around of uint32, the chunking of k_exclusive_scan at
every size around the workgroup's, widening, aliasing, and the total that is or is not written.  Lanes run one after another
here: that the shuffles and barriers of the device do the same is established by the GPU tests of the callers."""
import ctypes as C

import numpy as np
import pytest

import lanes
from lanes import p as _p

THREADS = (64, 256, 1024)
BLOCK_TYPES = {"int": (0, np.int32), "uint32": (1, np.uint32), "longlong": (2, np.int64)}
SCAN_TYPES = {"int32_to_int64": (0, np.int32, np.int64, False), "int_in_place": (1, np.int32, np.int32, True),
              "uint32_in_place": (2, np.uint32, np.uint32, True)}
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "scan_on_host.cpp")


def _values(rng, dtype, n, widening=False):
    if dtype == np.uint32:                                   # the whole range: the sums wrap
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if widening:                                             # counts whose sum passes 2^32: a sum kept in the input type would show
        return rng.integers(2 ** 30, 2 ** 31, n).astype(np.int32)
    return rng.integers(-1000, 1001, n).astype(dtype)        # both signs, no signed overflow


def _exclusive(values, dtype):
    """(exclusive prefix sums, total) of `values`, summed in `dtype` by numpy.cumsum."""
    with np.errstate(over="ignore"):
        inc = np.cumsum(values, dtype=dtype)
    return np.concatenate([np.zeros(1, dtype), inc[:-1]])[:len(values)], (inc[-1] if len(values) else dtype(0))


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("name", sorted(BLOCK_TYPES))
def test_block_functions_equal_cumsum_on_two_calls_in_a_row(emu, threads, name):
    lib, _ = emu
    code, dtype = BLOCK_TYPES[name]
    rng = np.random.default_rng(threads + code)
    src = np.stack([_values(rng, dtype, threads), _values(rng, dtype, threads)])
    if dtype == np.uint32:
        assert int(src[0].astype(np.uint64).sum()) >= 2 ** 32 and int(src[1][:64].astype(np.uint64).sum()) >= 2 ** 32   # the case wraps
    out = np.full((6, threads), SENTINEL, dtype)
    lanes.check(lib, lib.emu_scan_block(threads, code, _p(src), _p(out)))
    for half in range(2):
        prefix, total = _exclusive(src[half], dtype)
        assert np.array_equal(out[2 * half], prefix), np.flatnonzero(out[2 * half] != prefix)[:8]
        assert (out[2 * half + 1] == total).all() and (out[4 + half] == total).all()


@pytest.mark.parametrize("write_total", (0, 1))
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("name", sorted(SCAN_TYPES))
def test_scan_kernel_equals_cumsum(emu, threads, name, write_total):
    lib, _ = emu
    code, d_in, d_out, in_place = SCAN_TYPES[name]
    rng = np.random.default_rng(1000 * threads + 10 * code + write_total)
    for n in (0, 1, threads - 1, threads, threads + 1, 3 * threads + 5, 40 * threads + 3):
        src = _values(rng, d_in, n, widening=not in_place)
        prefix, total = _exclusive(src, d_out)
        out = np.full(n + 1, SENTINEL, d_out)
        if in_place:
            out[:n] = src
        lanes.check(lib, lib.emu_scan_kernel(threads, code, C.c_int64(n), _p(out if in_place else src), _p(out), write_total))
        assert np.array_equal(out[:n], prefix), (n, np.flatnonzero(out[:n] != prefix)[:8])
        assert out[n] == (total if write_total else SENTINEL), n          # out[n] is the total, or untouched


def test_sanitized_stand_alone_program(tmp_path):
    """The same sizes and types with a main of their own under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    host program: every array has its exact size (n elements where no total is asked for, so a write of out[n] is caught) and the
    results are checked against a serial loop inside the program."""
    stdout = lanes.sanitized(tmp_path, "scan_on_host.cpp", "SCAN_ON_HOST_MAIN")
    w = stdout.split()
    assert w[0] == "cases" and int(w[1]) == 3 * (3 + 7 * 2 * 3) and w[2] == "wrong" and int(w[3]) == 0, stdout
