"""The source of the cloud kernels, run lane by lane on the CPU: csrc/pxr_cloud.hip is compiled as host C++ over the stand-in
runtime of tests/lane_emulation and held to the brute-force statement of tests/cloud_cases.py bit for bit, on every case of
the GPU test -- the cell coordinates and their hash, count / scan / fill of the buckets, the walk over the 27 cells with its
tie-break, the voxel keys, the compare-and-swap inserts with their probing, the fixed-point sums and the host-side validation are
checked without a GPU.  The host's float64 division is correctly rounded, as numpy's is; whether the device's is stays with
tests/test_cloud_gpu.py.  Lanes run one after another here: what the integer atomics do under real concurrency does too."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as cc
import lanes
from lanes import p as _p

SENTINEL = -7


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "cloud_on_host.cpp")


def _nearest(emu, ref, query, max_dist, n_ref=None, n_query=None):
    lib, ctx = emu
    ref, query = np.ascontiguousarray(ref, np.float64), np.ascontiguousarray(query, np.float64)
    index, dist2 = np.full(max(len(query), 1), SENTINEL, np.int32), np.full(max(len(query), 1), float(SENTINEL))
    code = lib.pxr_cloud_nearest(ctx, C.c_int64(len(ref) if n_ref is None else n_ref), _p(ref), C.c_int64(len(query) if n_query is None else n_query),
                                 _p(query), C.c_double(max_dist), _p(index), _p(dist2))
    return code, index[:len(query)], dist2[:len(query)]


def _voxels(emu, xyz, dist2, voxel_size, tol, n=None, n_tol=None):
    lib, ctx = emu
    xyz, dist2, tol = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(dist2, np.float64), np.ascontiguousarray(tol, np.float64)
    frac, n_vox = np.full(max(len(tol), 1), float(SENTINEL)), C.c_int64(SENTINEL)
    code = lib.pxr_cloud_voxel_fractions(ctx, C.c_int64(len(xyz) if n is None else n), _p(xyz), _p(dist2), C.c_double(voxel_size),
                                         C.c_int32(len(tol) if n_tol is None else n_tol), _p(tol), _p(frac), C.byref(n_vox))
    return code, frac[:len(tol)], n_vox.value


@pytest.mark.parametrize("name", sorted(cc.NEAREST_CASES))
def test_nearest_equals_the_brute_force_search(emu, name):
    ref, query, max_dist = cc.NEAREST_CASES[name]
    code, index, dist2 = _nearest(emu, ref, query, max_dist)
    assert code == 0, emu[0].emu_last_error()
    r_index, r_dist2 = cc.nearest_reference(name)
    assert np.array_equal(index, r_index), np.flatnonzero(index != r_index)[:8]
    assert dist2.tobytes() == r_dist2.tobytes()


@pytest.mark.parametrize("name", sorted(cc.VOXEL_CASES))
def test_voxel_fractions_equal_the_reference(emu, name):
    xyz, dist2, v, tol = cc.VOXEL_CASES[name]
    code, frac, n_vox = _voxels(emu, xyz, dist2, v, tol)
    ref = cc.voxel_reference(name)
    if ref is None:                                                    # a voxel component of 2^20 or more: refused after the launch
        assert code == -1 and (frac == SENTINEL).all() and n_vox == SENTINEL
        assert b"2^20" in emu[0].emu_last_error()
        return
    assert code == 0, emu[0].emu_last_error()
    assert n_vox == ref[1]
    if ref[1] == 0:
        assert np.isnan(frac).all()
    else:
        assert frac.tobytes() == ref[0].tobytes(), (frac, ref[0])


def test_bad_arguments_are_refused_and_leave_the_outputs_untouched(emu):
    ref, query, _ = cc.NEAREST_CASES["size_65x64"]
    for kw in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=np.inf), dict(max_dist=np.nan), dict(n_ref=-1), dict(n_query=-1),
               dict(n_ref=2 ** 31), dict(n_query=2 ** 31)):
        code, index, dist2 = _nearest(emu, ref, query, **dict(dict(max_dist=0.1), **kw))
        assert code == -1 and (index == SENTINEL).all() and (dist2 == SENTINEL).all(), kw
    xyz, dist2, v, tol = cc.VOXEL_CASES["faces"]
    for kw in (dict(voxel_size=-1.0), dict(voxel_size=np.inf), dict(voxel_size=np.nan), dict(tol=[0.01, 0.0]), dict(tol=[np.inf]),
               dict(tol=[np.nan, 0.1]), dict(tol=[-0.1]), dict(n_tol=0), dict(tol=[0.1] * 9), dict(n=-1), dict(n=2 ** 30)):
        args = dict(dict(voxel_size=v, tol=tol), **kw)
        code, frac, n_vox = _voxels(emu, xyz, dist2, args.pop("voxel_size"), args.pop("tol"), **args)
        assert code == -1 and (frac == SENTINEL).all() and n_vox == SENTINEL, kw


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: both entry points on lattice clouds with rows that are not valid, checked
    against the brute-force search inside the program."""
    for args in (("300", "257", "0.25", "0.5"), ("65", "64", "1", "0"), ("1", "1", "0.1", "0.1"), ("0", "5", "0.1", "0.1"), ("4100", "70", "0.5", "0.25")):
        stdout = lanes.sanitized(tmp_path, "cloud_on_host.cpp", "CLOUD_ON_HOST_MAIN", *args)
        w = stdout.split()
        queries, found, wrong, voxels = int(w[1]), int(w[3]), int(w[5]), int(w[7])
        assert queries == int(args[1]) and wrong == 0 and 0 <= found <= queries and 0 <= voxels <= queries, stdout
        if int(args[0]) >= 300:
            assert found > 0, stdout
