"""The source of the triangulation kernels, run lane by lane on the CPU: csrc/pxr_triangulate.hip is compiled as host C++
over the stand-in runtime of tests/lane_emulation (a fibre per lane; the cross-lane operations of a 16-lane group) and
held to the numpy reference like the GPU test does -- the estimator's logic, the lane-strided loops, the chunk rotation of the
acceptance step, the compaction and the host-side validation are checked without a GPU.  What only hardware can show (DPP and
LDS behaviour, occupancy) stays with tests/test_triangulation_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import pxo
import triangulation_cases as tc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "triangulate_on_host.cpp")


def _run(emu, scene, xyz=None):
    from pixsfm_amd import _lib
    from pixsfm_amd.engine import _padded_cam_params, tri_options
    lib, ctx = emu
    off, oi = np.ascontiguousarray(scene["track_offsets"], np.int64), np.ascontiguousarray(scene["obs_image"], np.int32)
    xy, ic = np.ascontiguousarray(scene["obs_xy"], np.float64), np.ascontiguousarray(scene["image_camera"], np.int32)
    q, t = np.ascontiguousarray(scene["qvec"], np.float64), np.ascontiguousarray(scene["tvec"], np.float64)
    cm = np.ascontiguousarray(scene["cam_model"], np.int32)
    cp = _padded_cam_params(scene["cam_params"], len(cm))
    T, N = len(off) - 1, len(oi)
    view = _lib.TriView(T, _p(off), N, _p(oi), _p(xy), len(ic), _p(ic), _p(q), _p(t), len(cm), _p(cm), _p(cp))
    opts = tri_options()
    X = np.full((T, 3), np.nan) if xyz is None else np.array(xyz, dtype=np.float64)
    st, ni = np.full(T, -9, np.int32), np.full(T, -9, np.int32)
    inl, err = np.full(N, 9, np.uint8), np.full(N, -1.0)
    rc = lib.pxr_triangulate_tracks(ctx, C.byref(view), C.byref(opts), _p(X), _p(st), _p(ni), _p(inl), _p(err))
    lanes.check(lib, rc)
    return dict(xyz=X, status=st, n_inliers=ni, obs_inlier=inl, obs_err=err)


def _compare(got, ref, scene):
    assert (ref["margin"] >= 1e-9).all()
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["obs_inlier"], ref["obs_inlier"])
    ok = ref["status"] == 0
    assert np.abs(got["xyz"][ok] - ref["xyz"][ok]).max() <= 1e-9 and np.isnan(got["xyz"][~ok]).all()
    assert np.array_equal(np.isnan(got["obs_err"]), np.isnan(ref["obs_err"]))
    have = ~np.isnan(ref["obs_err"])
    assert np.abs(got["obs_err"][have] - ref["obs_err"][have]).max() <= 1e-7


def test_undistortion_source_inverts_all_models(emu):
    lib, ctx = emu
    grid, models = tc.polar_grid(), sorted(tc.MODEL_PARAMS)
    uv0 = np.tile(grid, (len(models), 1))
    cam = np.repeat(np.arange(len(models), dtype=np.int32), len(grid))
    xy = np.array([pxo.world_to_image(models[c], np.array(tc.MODEL_PARAMS[models[c]]), u, v)[0] for c, (u, v) in zip(cam, uv0)])
    bad = [70, 300, len(xy) - 1]
    xy[bad[0], 0] = np.nan; xy[bad[1], 1] = np.nan; xy[bad[2]] = np.inf
    cm, cp = np.array(models, np.int32), tc.pad_params([tc.MODEL_PARAMS[m] for m in models])
    uv, ok = np.zeros_like(xy), np.full(len(xy), 9, np.uint8)
    assert lib.pxr_image_to_world(ctx, C.c_int64(len(xy)), _p(cam), len(cm), _p(cm), _p(cp), _p(xy), _p(uv), _p(ok)) == 0
    good = np.setdiff1d(np.arange(len(xy)), bad)
    assert ok[good].all() and np.abs(uv - uv0)[good].max() <= 1e-12
    assert not ok[bad].any() and np.isnan(uv[bad]).all()


def test_kernel_source_matches_the_reference(emu):
    # track lengths around the 16-lane group (15, 16, 17), past the LDS staging limit (33, 40) and past the hypothesis cap (24, 33, 40)
    lengths = np.array([0, 1, 2, 3, 5, 15, 16, 17, 23, 24, 33, 40] * 3 + [4, 7])
    scene = tc.make_scene(lengths, n_cams=48, models=(2, 1, 8), seed=6)
    scene["obs_xy"][scene["track_offsets"][4] + 2] = np.nan                    # an observation that cannot be undistorted
    ref = tc.reference(scene)
    assert len(lengths) % 4 != 0 and {0, 1}.issubset(set(ref["status"]))
    _compare(_run(emu, scene), ref, scene)


def test_status_codes_and_validation(emu):
    scene = tc.status_scene()
    sentinel = np.arange(9.0).reshape(3, 3) - 100
    got = _run(emu, scene, xyz=sentinel)
    assert got["status"].tolist() == [1, 2, 3] and got["n_inliers"].tolist() == [0, 0, 0] and np.array_equal(got["xyz"], sentinel)
    assert not got["obs_inlier"].any() and np.isnan(got["obs_err"]).all()
    for change, word in ((dict(track_offsets=np.array([0, 3, 1, 6], np.int64)), "monotone"),
                         (dict(track_offsets=np.array([0, 1, 3, 5], np.int64)), "n_obs"),
                         (dict(obs_image=np.array([0, 0, 1, 0, 3, 2], np.int32)), "image"),
                         (dict(image_camera=np.array([0, 1, 0], np.int32)), "camera")):
        with pytest.raises(ValueError, match=word):
            _run(emu, dict(scene, **change))
