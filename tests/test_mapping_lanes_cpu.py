"""The source of the mapper's visibility kernels, run lane by lane on the CPU: csrc/pxr_mapper.hip is compiled as host C++ over the
stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through
an exchange buffer) and held bit for bit to the numpy reference of tests/mapping_cases.py on the shapes of the GPU test -- the
occupancy words, the workgroup sums, the prefix sums across the four wavefronts and the chunks of a long image, and the host-side
validation are checked without a GPU.  What only hardware can show (LDS atomics under contention, the device's floor and division)
stays with tests/test_mapping_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import mapping_cases as mc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "mapping_on_host.cpp")


def _run(emu, scene, xyz, status, mask, levels, **replace):
    """The C entry point on host arrays; replace: arrays by the keys of MapperScene.d.  Returns (outputs with sentinels where
    nothing was written, n_corr)."""
    from pixsfm_amd import _lib
    from pixsfm_amd.engine import MapperScene
    lib, ctx = emu
    s = MapperScene(None, scene)
    a = dict(track_offsets=s.track_offsets, obs_image=s.obs_image, obs_xy=s.obs_xy, obs_track=s.obs_track,
             image_obs_offsets=s.image_obs_offsets, image_obs=s.image_obs, image_camera=s.image_camera, cam_size=s.cam_size)
    for k, v in replace.items():
        a[k] = np.ascontiguousarray(v, dtype=a[k].dtype)
    xyz, status = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(status, np.int32)
    mask = np.ascontiguousarray(mask, np.uint8)
    view = _lib.TriView(s.n_tracks, a["track_offsets"].ctypes.data, s.n_obs, a["obs_image"].ctypes.data, a["obs_xy"].ctypes.data,
                        s.n_images, a["image_camera"].ctypes.data, None, None, s.n_cameras, None, None)
    out = dict(n_visible=np.full(s.n_images, -9, np.int32), score=np.full(s.n_images, -9, np.int64),
               corr_offsets=np.full(s.n_images + 1, -9, np.int64), corr_obs=np.full(s.n_obs, -9, np.int64),
               corr_xy=np.full((s.n_obs, 2), -9.0), corr_xyz=np.full((s.n_obs, 3), -9.0))
    n_corr = C.c_int64(-9)
    rc = lib.pxr_mapper_visibility(ctx, C.byref(view), _p(a["obs_track"]), _p(a["image_obs_offsets"]), _p(a["image_obs"]), _p(xyz),
                                   _p(status), _p(mask), _p(a["cam_size"]), C.c_int32(levels), _p(out["n_visible"]), _p(out["score"]),
                                   _p(out["corr_offsets"]), _p(out["corr_obs"]), _p(out["corr_xy"]), _p(out["corr_xyz"]),
                                   C.byref(n_corr))
    try:
        lanes.check(lib, rc)
    except ValueError as err:
        err.outputs, err.n_corr = out, n_corr.value
        raise
    return out, n_corr.value


def _equal(got, n_corr, ref):
    assert n_corr == ref["n_corr"]
    for k in ("n_visible", "score", "corr_offsets"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("corr_obs", "corr_xy", "corr_xyz"):
        assert np.array_equal(got[k][:n_corr], ref[k], equal_nan=False), k
        assert (got[k][n_corr:] == -9).all(), k + ": written past n_corr"


@pytest.mark.parametrize("levels", [1, 6])
def test_kernel_source_matches_the_reference_on_the_boundary_batch(emu, levels):
    scene, xyz, status, mask, planned = mc.boundary_batch()
    ref = mc.visibility_reference(scene, xyz, status, mask, levels)
    assert ref["n_visible"].tolist() == planned.tolist()
    got, n_corr = _run(emu, scene, xyz, status, mask, levels)
    _equal(got, n_corr, ref)


@pytest.mark.parametrize("n_images", [257, 600])
def test_offsets_over_many_images_match_the_reference(emu, n_images):
    """More images than the prefix sum over their counts has threads: two and three images to a thread."""
    scene, xyz, status, mask = mc.many_images_batch(n_images)
    got, n_corr = _run(emu, scene, xyz, status, mask, 3)
    _equal(got, n_corr, mc.visibility_reference(scene, xyz, status, mask, 3))


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(emu):
    scene, xyz, status, mask, _ = mc.boundary_batch()
    for name, key, bad, word in mc.bad_inputs(scene):
        with pytest.raises(ValueError, match=word) as e:
            _run(emu, scene, xyz, status, mask, 6, **{key: bad})
        assert e.value.args[0].startswith("-1:"), name                     # PXR_EINVAL
        assert all((v == -9).all() for v in e.value.outputs.values()) and e.value.n_corr == -9, name
    for levels in (0, 7):
        with pytest.raises(ValueError, match="pyramid_levels"):
            _run(emu, scene, xyz, status, mask, levels)


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: images of 0, 1, 63, 64, 65, 256, 257 and 600 observations, a third of the tracks
    without a point, a seventh of the keypoints not finite, one image masked out."""
    counts = [65, 300, 0, 1, 63, 64, 256, 257, 600]
    stdout = lanes.sanitized(tmp_path, "mapping_on_host.cpp", "MAPPING_ON_HOST_MAIN", *counts)
    for levels in (1, 6):
        rows = [ln.split() for ln in stdout.split("\n") if ln.startswith("L %d image" % levels)]
        assert [int(r[5]) for r in rows] == counts
        visible, score, offset = ([int(r[k]) for r in rows] for k in (7, 9, 11))
        assert visible[1] == 0 and score[1] == 0 and visible[2] == 0                               # masked out; empty
        assert all(0 < v < c for v, c in zip(visible[3:], counts[3:]) if c >= 63)                  # some visible, some not
        assert offset == np.concatenate([[0], np.cumsum(visible)[:-1]]).tolist()
        assert ("L %d total %d" % (levels, sum(visible))) in stdout
        assert all(s <= sum(4 ** l for l in range(1, levels + 1)) * v for s, v in zip(score, visible))
