"""Generates tests/golden/half_ref_outputs.npz: what the REFERENCE's vendored third-party/half.hpp (compiled from its own source
into oracle/_ref/libpxo_ref_half.so, oracle/ref_half_shim.cc) returns for the exact inputs of
  tests/test_oracle_costmap.py  test_half_subtraction_rule_matches_reference_half_hpp  (key "sub":         half - half)
                                test_set_entry_cast_rule_matches_reference_half_hpp  (key "from_double": dtype(double))
  tests/test_oracle_interp.py   test_half_widening_matches_the_references_half_hpp   (key "to_float":    every binary16 pattern)
stored as XOR against numpy's plain conversion, with a digest of each input (tests/half_ref.py), so that those tests run where
oracle/_ref cannot be built.

Needs oracle/_ref (make -C oracle with a reference checkout at REF):  python tests/golden/make_golden_half_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "pixel-perfect-sfm_amd")):
    sys.path.insert(0, p)
import half_ref  # noqa: E402
import test_oracle_costmap  # noqa: E402

inputs = {"sub": (test_oracle_costmap.half_sub_inputs(), np.float16),
          "from_double": (test_oracle_costmap.half_from_double_inputs(), np.uint16),
          "to_float": ((np.arange(65536, dtype=np.uint16),), np.float32)}
out = {}
for key, (args, dtype) in inputs.items():
    got = half_ref.live(key, args, dtype)
    assert got is not None, "build oracle/_ref first (make -C oracle)"
    out[key] = half_ref.encode(key, args, got)
    out[key + "_digest"] = np.array(half_ref.digest(*args))
np.savez_compressed(half_ref.GOLDEN, **out)
print("wrote", half_ref.GOLDEN, os.path.getsize(half_ref.GOLDEN), "bytes")
