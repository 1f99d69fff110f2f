"""The reference's vendored third-party/half.hpp on the tests' own inputs.

Live through oracle/_ref/libpxo_ref_half.so where that library was built (oracle/Makefile builds it from the reference's own
source when a reference checkout is at hand); everywhere else from the outputs it gave for the same inputs, stored in
tests/golden/half_ref_outputs.npz by tests/golden/make_golden_half_ref.py.  The stored file carries a digest of each input, so a
changed input fails loudly instead of being compared with another input's output; where the library is built, its output must
also equal the stored one."""
import ctypes as C
import hashlib
import os

import numpy as np

import pxo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "half_ref_outputs.npz")
# key -> entry point of oracle/ref_half_shim.cc: (inputs..., out, n)
ENTRIES = {"sub": "pxo_ref_half_sub", "from_double": "pxo_ref_half_from_double", "to_float": "pxo_ref_half_to_float"}
# the file stores half.hpp's output bits XOR those of numpy's plain conversion of the same inputs (mostly zero: 5 KB instead of
# 1.4 MB); the baseline is numpy alone, never the oracle under test
BASELINE = {"sub": lambda a, b: (a.astype(np.float32) - b.astype(np.float32)).astype(np.float16),
            "from_double": lambda v: v.astype(np.float16),
            "to_float": lambda bits: bits.view(np.float16).astype(np.float32)}
UINT = {2: np.uint16, 4: np.uint32}


def encode(key, inputs, out):
    base = BASELINE[key](*inputs)
    return out.view(UINT[out.itemsize]) ^ base.view(UINT[out.itemsize])


def decode(key, inputs, stored, out_dtype):
    base = BASELINE[key](*inputs)
    return (stored ^ base.view(UINT[out_dtype.itemsize])).view(out_dtype)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def live(key, inputs, out_dtype):
    """half.hpp's output through oracle/_ref, or None where that library is not built."""
    r = pxo.ref()
    if r is None or not hasattr(r, ENTRIES[key]):
        return None
    out = np.empty(inputs[0].size, out_dtype)
    getattr(r, ENTRIES[key])(*[np.ascontiguousarray(a).ctypes.data_as(C.c_void_p) for a in inputs],
                             out.ctypes.data_as(C.c_void_p), C.c_int64(out.size))
    return out


def run(key, inputs, out_dtype):
    """half.hpp's output for `inputs`: live where oracle/_ref is built (and then equal to the stored one), else the stored one."""
    out_dtype = np.dtype(out_dtype)
    got = live(key, inputs, out_dtype)
    g = np.load(GOLDEN) if (got is None or os.path.exists(GOLDEN)) else None
    if g is not None:
        assert str(g[key + "_digest"]) == digest(*inputs), \
            "the inputs of %r differ from those stored in %s (tests/golden/make_golden_half_ref.py)" % (key, GOLDEN)
        stored = decode(key, inputs, g[key], out_dtype)
        if got is None:
            return stored
        assert np.array_equal(got.view(np.uint8), stored.view(np.uint8)), "%s is out of date for %r" % (GOLDEN, key)
    return got
