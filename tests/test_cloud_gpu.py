"""GPU: the cloud kernels (csrc/pxr_cloud.hip) against the brute-force statement of tests/cloud_cases.py, bit for bit: indices and
voxel counts with array_equal, squared distances and fractions as bytes.  The reference's float64 operations are numpy's,
correctly rounded and never fused; that the device's division, floor and llrint give those bits, and that the integer atomics
of thousands of concurrent lanes build the same tables, is what these tests establish."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as cc

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _nearest(ctx, ref, query, max_dist):
    from pixsfm_amd.engine import cloud_nearest
    index, dist2 = cloud_nearest(ctx, ref, query, max_dist)
    return index.download(), dist2.download()


@pytest.mark.parametrize("name", sorted(cc.NEAREST_CASES))
def test_nearest_equals_the_brute_force_search(ctx, name):
    ref, query, max_dist = cc.NEAREST_CASES[name]
    index, dist2 = _nearest(ctx, ref, query, max_dist)
    r_index, r_dist2 = cc.nearest_reference(name)
    assert index.dtype == np.int32 and dist2.dtype == np.float64
    assert np.array_equal(index, r_index), np.flatnonzero(index != r_index)[:8]
    assert dist2.tobytes() == r_dist2.tobytes()
    index2, dist22 = _nearest(ctx, ref, query, max_dist)               # two runs give identical bits
    assert index2.tobytes() == index.tobytes() and dist22.tobytes() == dist2.tobytes()


def test_nearest_with_more_scan_chunks_than_scan_threads(ctx):
    """The bucket table is one scan chunk in the size_* cases and two in random_3000x2000, one_cell and spread; here it is 512, so
    that the one workgroup over the chunks' totals (k_exclusive_scan<256> of csrc/pxr_scan.h, in place) gives two to a thread."""
    ref, query, max_dist = cc.many_chunks_case()
    index, dist2 = _nearest(ctx, ref, query, max_dist)
    r_index, r_dist2 = cc.nearest(ref, query, max_dist)
    assert (r_index >= 0).sum() > 32
    assert np.array_equal(index, r_index), np.flatnonzero(index != r_index)[:8]
    assert dist2.tobytes() == r_dist2.tobytes()


def test_pairs_at_exactly_max_dist(ctx):
    for s in cc.EXACT_SCALES:
        for name, (ref, query, max_dist, inside) in cc.exact_pairs(s).items():
            index, dist2 = _nearest(ctx, ref, query, max_dist)
            assert (index[inside] >= 0).all() and (dist2[inside] == max_dist * max_dist).all(), name
            assert (index[~inside] == -1).all() and np.isposinf(dist2[~inside]).all(), name


def test_device_arrays_are_used_in_place(ctx):
    from pixsfm_amd.engine import cloud_nearest, cloud_voxel_fractions
    ref, query, max_dist = cc.NEAREST_CASES["random_3000x2000"]
    d_ref, d_query = ctx.to_device(ref, np.float64), ctx.to_device(query, np.float64)
    index, dist2, ms = cloud_nearest(ctx, d_ref, d_query, max_dist, timed=True)
    assert set(ms) == {"grid", "query"} and all(v >= 0 for v in ms.values())
    r_index, r_dist2 = cc.nearest_reference("random_3000x2000")
    assert np.array_equal(index.download(), r_index) and dist2.download().tobytes() == r_dist2.tobytes()
    frac, n_vox, ms = cloud_voxel_fractions(ctx, d_query, dist2, 0.05, cc.TOL3, timed=True)
    assert set(ms) == {"insert", "reduce"}
    r_frac, r_n = cc.voxel_fractions(query, r_dist2, 0.05, cc.TOL3)
    assert n_vox == r_n and frac.tobytes() == r_frac.tobytes()


@pytest.mark.parametrize("name", sorted(cc.VOXEL_CASES))
def test_voxel_fractions_equal_the_reference(ctx, name):
    from pixsfm_amd._lib import PixsfmHipError
    from pixsfm_amd.engine import cloud_voxel_fractions
    xyz, dist2, v, tol = cc.VOXEL_CASES[name]
    ref = cc.voxel_reference(name)
    if ref is None:                                                    # a voxel component of 2^20 or more: refused after the launch
        d_x, d_d = ctx.to_device(xyz, np.float64), ctx.to_device(dist2, np.float64)
        t = np.ascontiguousarray(tol, np.float64)
        frac, n_vox = np.full(len(t), float(SENTINEL)), C.c_int64(SENTINEL)
        code = ctx.lib.pxr_cloud_voxel_fractions(ctx.handle, len(xyz), d_x.ptr, d_d.ptr, v, len(t), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                 frac.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_vox))
        assert code == -1 and (frac == SENTINEL).all() and n_vox.value == SENTINEL
        with pytest.raises(PixsfmHipError, match="2\\^20"):
            cloud_voxel_fractions(ctx, xyz, dist2, v, tol)
        return
    frac, n_vox = cloud_voxel_fractions(ctx, xyz, dist2, v, tol)
    assert n_vox == ref[1]
    if ref[1] == 0:
        assert np.isnan(frac).all()
    else:
        assert frac.tobytes() == ref[0].tobytes(), (frac, ref[0])
    frac2, n_vox2 = cloud_voxel_fractions(ctx, xyz, dist2, v, tol)     # two runs give identical bits
    assert n_vox2 == n_vox and frac2.tobytes() == frac.tobytes()


def test_bad_arguments_are_refused_and_leave_the_outputs_untouched(ctx):
    ref, query, _ = cc.NEAREST_CASES["size_65x64"]
    d_ref, d_query = ctx.to_device(ref, np.float64), ctx.to_device(query, np.float64)
    d_index = ctx.to_device(np.full(len(query), SENTINEL, np.int32), np.int32)
    d_dist2 = ctx.to_device(np.full(len(query), float(SENTINEL)), np.float64)
    for kw in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=np.inf), dict(max_dist=np.nan), dict(n_ref=-1), dict(n_query=-1),
               dict(n_ref=2 ** 31), dict(n_query=2 ** 31)):
        a = dict(dict(max_dist=0.1, n_ref=len(ref), n_query=len(query)), **kw)
        code = ctx.lib.pxr_cloud_nearest(ctx.handle, a["n_ref"], d_ref.ptr, a["n_query"], d_query.ptr, a["max_dist"], d_index.ptr, d_dist2.ptr)
        assert code == -1, kw
    assert (d_index.download() == SENTINEL).all() and (d_dist2.download() == SENTINEL).all()

    xyz, dist2, v, tol = cc.VOXEL_CASES["faces"]
    d_x, d_d = ctx.to_device(xyz, np.float64), ctx.to_device(dist2, np.float64)
    for kw in (dict(v=-1.0), dict(v=np.inf), dict(v=np.nan), dict(tol=[0.01, 0.0]), dict(tol=[np.inf]), dict(tol=[np.nan, 0.1]), dict(tol=[-0.1]),
               dict(n_tol=0), dict(tol=[0.1] * 9), dict(n=-1), dict(n=2 ** 30)):
        a = dict(dict(v=v, tol=tol, n=len(xyz)), **kw)
        t = np.ascontiguousarray(a["tol"], np.float64)
        frac, n_vox = np.full(len(t), float(SENTINEL)), C.c_int64(SENTINEL)
        code = ctx.lib.pxr_cloud_voxel_fractions(ctx.handle, a["n"], d_x.ptr, d_d.ptr, a["v"], a.get("n_tol", len(t)),
                                                 t.ctypes.data_as(C.POINTER(C.c_double)), frac.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_vox))
        assert code == -1 and (frac == SENTINEL).all() and n_vox.value == SENTINEL, kw
