"""Generates tests/golden/shim_bindings_ref.json: the names the REFERENCE's pybind11 modules bind (pixsfm/*/bindings.cc), as
tests/test_shim_surface.py parses them (bound_names) -- module-level classes / functions / attributes and the methods /
properties of each bound class -- so that the surface test runs without the reference tree.  Data only: names, no source.

    python tests/golden/make_golden_bindings.py <pixel-perfect-sfm checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_shim_surface as t  # noqa: E402

ref = os.path.join(sys.argv[1], "pixsfm")
out = {mod_name: t.bound_names(open(os.path.join(ref, rel)).read()) for mod_name, rel in t.BINDINGS.items()}
with open(t.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", t.GOLDEN, os.path.getsize(t.GOLDEN), "bytes")
