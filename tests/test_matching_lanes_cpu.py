"""The source of the matching kernels, run lane by lane on the CPU: csrc/pxr_match.hip is compiled as host C++ over a stand-in
runtime (tests/lane_emulation/matrix: the workgroup stand-in plus the f32-input MFMA stated as its documented lane maps and fmaf
chain) and held to the reference of tests/matching_cases.py bit for bit, like the GPU test does -- the fragment order of the LDS
tiles, the masks at the tile edges, the running and merged top-2, the partials across strips, the mutual check and the host-side
validation are checked without a GPU.  Whether the hardware instruction computes that chain stays with tests/test_matching_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import matching_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "lane_emulation")


def _clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cand = [os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
            shutil.which("clang++")]
    return next((c for c in cand if c and os.path.exists(c)), None)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = _clang()       # the kernels use clang's vector types: the compiler that hipcc drives, as a plain host compiler
    assert cxx, "no clang++ next to hipcc"
    out = str(tmp_path_factory.mktemp("lanes") / "libmatch_lanes.so")
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I", os.path.join(HERE, "matrix"), "-I", HERE, "-I", os.path.join(ROOT, "pixel-perfect-sfm_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "match_on_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_ctx.restype = C.c_void_p
    lib.emu_last_error.restype = C.c_char_p
    return lib, C.c_void_p(lib.emu_ctx())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(emu, descs, pairs, offsets=None, dim=None, **options):
    from pixsfm_amd.engine import match_options
    lib, ctx = emu
    dim = descs[0].shape[1] if dim is None else dim
    desc = np.ascontiguousarray(np.concatenate(descs), np.float32)
    off = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    sizes = [len(descs[a]) if 0 <= a < len(descs) else 0 for a, _ in pairs]
    poff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    m, s, n = np.full(poff[-1], -7, np.int32), np.full(poff[-1], -7.0, np.float32), np.full(len(pairs), -7, np.int32)
    opts = match_options(**options)
    rc = lib.pxr_match_descriptors(ctx, C.c_int32(len(descs)), _p(off), C.c_int64(len(desc)), C.c_int32(dim), _p(desc), C.c_int32(len(pairs)),
                                   _p(pairs), _p(poff), C.byref(opts), _p(m), _p(s), _p(n))
    if rc:
        raise ValueError("%d: %s" % (rc, lib.emu_last_error().decode()))
    return m, s, n


def _equal(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, np.flatnonzero(got[0] != ref[0])[:8])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (what, np.flatnonzero(got[1] != ref[1])[:8])
    assert np.array_equal(got[2], ref[2]), (what, got[2], ref[2])


@pytest.mark.parametrize("shape", [s for s in mc.GPU_SHAPES if s != (300, 200, 256)] + [(130, 40, 258)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_source_equals_the_reference(emu, shape):
    A, B = mc.pair_case(*shape, seed=100 + (mc.GPU_SHAPES.index(shape) if shape in mc.GPU_SHAPES else 50))
    sim = mc.sim_chain(A, B)
    for name, options in mc.OPTION_SETS.items():
        rm, rs, rn = mc.match_from_sim(sim, **options)
        _equal(_run(emu, [A, B], [(0, 1)], **options), (rm, rs, np.array([rn], np.int32)), "%s %s" % (shape, name))


def test_ties_and_the_batch(emu):
    for copies_in_b in (True, False):
        A, B = mc.tie_case(copies_in_b)
        for name in ("NN-mutual", "NN-ratio"):
            rm, rs, rn = mc.match_reference(A, B, mc.CONFS[name])
            _equal(_run(emu, [A, B], [(0, 1)], **mc.CONFS[name]), (rm, rs, np.array([rn], np.int32)), "ties %s %s" % (copies_in_b, name))
    descs, pairs = mc.batch_case()
    for name in ("NN-ratio", "NN-ratio-one-way"):
        _equal(_run(emu, descs, pairs, **mc.OPTION_SETS[name]), mc.reference_batch(descs, pairs, mc.OPTION_SETS[name]), "batch " + name)


def test_validation(emu):
    descs = [mc.unit_rows(np.random.default_rng(8), n, 16) for n in (40, 50)]
    for change, word in ((dict(offsets=[1, 40, 90]), "d_image_offsets"), (dict(offsets=[0, 95, 90]), "monotone"),
                         (dict(offsets=[0, 40, 80]), "n_total"), (dict(pairs=[(0, 1), (1, 2)]), "d_pairs"), (dict(dim=0), "dim"),
                         (dict(dim=513), "dim")):
        kw = dict(pairs=[(0, 1), (1, 0)])
        kw.update(change)
        with pytest.raises(ValueError, match="pxr_match_descriptors.*" + word):
            _run(emu, descs, **kw)
    m, s, n = _run(emu, [descs[0][:0], descs[1][:0]], [(0, 1), (1, 1)])
    assert len(m) == 0 and n.tolist() == [0, 0]
