"""The source of the matching kernels, run lane by lane on the CPU: csrc/pxr_match.hip is compiled as host C++ over the stand-in
runtime of tests/lane_emulation (a fibre per lane, the f32-input MFMA stated as its documented lane maps and fmaf
chain) and held to the reference of tests/matching_cases.py bit for bit, like the GPU test does -- the fragment order of the LDS
tiles, the masks at the tile edges, the running and merged top-2, the partials across strips, the mutual check and the host-side
validation are checked without a GPU.  Whether the hardware instruction computes that chain stays with tests/test_matching_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import matching_cases as mc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "match_on_host.cpp")


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
    lanes.check(lib, rc)
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
