"""The source of the global-mapping kernels, run lane by lane on the CPU: csrc/pxr_global.hip is compiled as host C++ over the
stand-in runtime of tests/lane_emulation (with a plain host Cholesky in place of the library's) and held to the numpy references of
tests/global_mapping_cases.py on boundary_batch(): integer and status outputs equal, floating outputs within
global_mapping_cases.bound() -- 100 times the largest difference this test measured (it prints them), never more than 1e-6 of the
scene radius.  What only hardware can show (integer atomics under contention, the device's libm, the blocked Cholesky) stays with
tests/test_global_mapping_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import global_mapping_cases as gc
import lanes
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "global_on_host.cpp")


def run_rotavg(lib, ctx, n_images, pair_image, pair_qvec, pair_weight, check=lanes.check, **options):
    """pxr_rotation_averaging on host arrays -> dict like the reference's; the outputs start from sentinels, and a ValueError carries
    them as .outputs."""
    from pixsfm_amd.engine import rotavg_options
    pim = np.ascontiguousarray(pair_image, np.int32).reshape(-1, 2)
    pq, pw = np.ascontiguousarray(pair_qvec, np.float64), np.ascontiguousarray(pair_weight, np.float64)
    opts = rotavg_options(**options)
    out = dict(qvec=np.full((n_images, 4), -9.0), pair_angle=np.full(len(pim), -9.0))
    root, iterations = C.c_int32(-9), C.c_int32(-9)
    rc = lib.pxr_rotation_averaging(ctx, C.c_int32(n_images), C.c_int32(len(pim)), _p(pim), _p(pq), _p(pw), C.byref(opts), _p(out["qvec"]),
                                    C.byref(root), C.byref(iterations), _p(out["pair_angle"]))
    out.update(root=root.value, iterations=iterations.value)
    try:
        check(lib, rc)
    except Exception as err:
        err.outputs = out
        raise
    return out


def run_positioning(lib, ctx, scene, qvec, pair_image, pair_dir, pair_weight, root, check=lanes.check, **options):
    """pxr_global_positioning on host arrays -> dict like the reference's (xyz keeps its sentinel where nothing is written)."""
    from pixsfm_amd import _lib
    from pixsfm_amd.engine import _padded_cam_params, globalpos_options
    off = np.ascontiguousarray(scene["track_offsets"], np.int64)
    img, xy = np.ascontiguousarray(scene["obs_image"], np.int32), np.ascontiguousarray(scene["obs_xy"], np.float64)
    icam, model = np.ascontiguousarray(scene["image_camera"], np.int32), np.ascontiguousarray(scene["cam_model"], np.int32)
    params = _padded_cam_params(scene["cam_params"], len(model))
    q = np.ascontiguousarray(qvec, np.float64)
    pim = np.ascontiguousarray(pair_image, np.int32).reshape(-1, 2)
    pd, pw = np.ascontiguousarray(pair_dir, np.float64), np.ascontiguousarray(pair_weight, np.float64)
    T, N, n = len(off) - 1, len(img), len(icam)
    view = _lib.TriView(T, off.ctypes.data, N, img.ctypes.data, xy.ctypes.data, n, icam.ctypes.data, q.ctypes.data, None, len(model),
                        model.ctypes.data, params.ctypes.data)
    opts = globalpos_options(**options)
    out = dict(centre=np.full((n, 3), -9.0), xyz=np.full((T, 3), -9.0), track_status=np.full(T, -9, np.int32), obs_weight=np.full(N, -9.0),
               pair_weight=np.full(len(pim), -9.0))
    status, rounds = C.c_int32(-9), C.c_int32(-9)
    rc = lib.pxr_global_positioning(ctx, C.byref(view), C.c_int32(len(pim)), _p(pim), _p(pd), _p(pw), C.c_int32(int(root)), C.byref(opts),
                                    _p(out["centre"]), _p(out["xyz"]), _p(out["track_status"]), _p(out["obs_weight"]), _p(out["pair_weight"]),
                                    C.byref(status), C.byref(rounds))
    out.update(status=status.value, rounds=rounds.value)
    try:
        check(lib, rc)
    except Exception as err:
        err.outputs = out
        raise
    return out


@pytest.mark.parametrize("n_images", gc.LAPLACIAN_SIZES)
def test_rotation_averaging_source_matches_the_reference(emu, n_images):
    scene, ref, _, _ = gc.solved("boundary", n_images)
    got = run_rotavg(*emu, n_images, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    assert (got["qvec"][:, 0] >= 0).all() and np.allclose(np.linalg.norm(got["qvec"], axis=1), 1.0, atol=1e-14)
    gc.within_bounds(gc.compare_rotavg(got, ref))


@pytest.mark.parametrize("n_images", gc.POSITIONING_SIZES)
def test_positioning_source_matches_the_reference(emu, n_images):
    scene, ra, b, ref = gc.solved("boundary", n_images)
    sp = scene["special"]
    assert ref["track_status"][sp["parallel"]] == 1 and ref["track_status"][sp["twice"]] == 0            # what the batch was built for
    assert ref["track_status"][:len(gc.BOUNDARY_LENGTHS)].tolist() == [0] * len(gc.BOUNDARY_LENGTHS)
    assert ref["obs_weight"][sp["nan_obs"]] == 0 and ref["obs_weight"][sp["far_obs"]] < 1e-3
    assert np.isfinite(ref["centre"]).all() and np.linalg.norm(ref["centre"][sp["empty_image"]]) > 1.0   # positioned by its pairs alone
    got = run_positioning(*emu, scene, ra["qvec"], scene["pair_image"], b, scene["pair_weight"], ra["root"])
    gc.within_bounds(gc.compare_positioning(got, ref))


def test_a_degenerate_system_is_a_status_not_an_error(emu):
    """All pair weights zero: g = 0, so g . y is not positive -- status 1 with return value 0, as in the reference."""
    scene, ra, b, _ = gc.solved("boundary", 22)
    zero = np.zeros(len(b))
    ref = gc.global_positioning_reference(scene, ra["qvec"], scene["pair_image"], b, zero, ra["root"])
    got = run_positioning(*emu, scene, ra["qvec"], scene["pair_image"], b, zero, ra["root"])
    assert ref["status"] == 1 and got["status"] == 1 and got["rounds"] == 0


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(emu):
    scene, ra, b, _ = gc.solved("boundary", 22)
    n = len(scene["image_camera"])
    for name, key, bad, word in gc.bad_rotation_inputs(scene):
        a = dict(pair_image=scene["pair_image"], pair_qvec=scene["pair_qvec"], pair_weight=scene["pair_weight"])
        a[key] = bad
        if key == "pair_image" and len(bad) != len(scene["pair_image"]):
            a["pair_qvec"], a["pair_weight"] = scene["pair_qvec"][:len(bad)], scene["pair_weight"][:len(bad)]
            assert gc.rotation_averaging_reference(n, bad, a["pair_qvec"], a["pair_weight"]) is None
        with pytest.raises(ValueError, match=word) as e:
            run_rotavg(*emu, n, a["pair_image"], a["pair_qvec"], a["pair_weight"])
        assert e.value.args[0].startswith("-1:") and gc.untouched(e.value.outputs), name          # PXR_EINVAL
    with pytest.raises(ValueError, match="PXR_MAX_IMAGES_DIRECT") as e:
        run_rotavg(*emu, 1002, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    assert gc.untouched(e.value.outputs)
    for name, key, bad, word in gc.bad_positioning_inputs(scene, b):
        sc, a = dict(scene), dict(pair_image=scene["pair_image"], pair_dir=b, pair_weight=scene["pair_weight"], root=ra["root"])
        if key in a:
            a[key] = bad
        else:
            sc[key] = bad
        with pytest.raises(ValueError, match=word) as e:
            run_positioning(*emu, sc, ra["qvec"], a["pair_image"], a["pair_dir"], a["pair_weight"], a["root"])
        assert e.value.args[0].startswith("-1:") and gc.untouched(e.value.outputs), name
    # 1002 images: 3 (n - 1) = 3003 columns, one image beyond what the dense solve takes (1001 images are the largest size allowed)
    big = dict(scene, image_camera=np.zeros(1002, np.int32))
    with pytest.raises(ValueError, match="PXR_MAX_IMAGES_DIRECT") as e:
        run_positioning(*emu, big, np.tile([1.0, 0.0, 0.0, 0.0], (1002, 1)), scene["pair_image"], b, scene["pair_weight"], ra["root"])
    assert e.value.args[0].startswith("-1:") and gc.untouched(e.value.outputs)


def test_the_largest_size_is_1001_images(emu):
    """The limit sits where the header says: n_images - 1 = PXR_MAX_IMAGES_DIRECT = 1000 passes the size check of both entry points
    (and is refused for what comes next: images that nothing connects, an observation out of range), 1002 images do not."""
    scene, ra, b, _ = gc.solved("boundary", 22)
    with pytest.raises(ValueError, match="not connected") as e:
        run_rotavg(*emu, 1001, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    assert e.value.args[0].startswith("-1:") and gc.untouched(e.value.outputs)
    sc = dict(scene, image_camera=np.zeros(1001, np.int32), obs_image=np.full(len(scene["obs_image"]), 1001, np.int32))
    with pytest.raises(ValueError, match="image outside") as e:
        run_positioning(*emu, sc, np.tile([1.0, 0.0, 0.0, 0.0], (1001, 1)), scene["pair_image"], b, scene["pair_weight"], ra["root"])
    assert e.value.args[0].startswith("-1:") and gc.untouched(e.value.outputs)


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, every array at its exact
    size: 23 images (66 columns: one full Cholesky block and a remainder in the library; here the plain solve), tracks at the edges
    of the 16-lane group and one far longer than the ring."""
    stdout = lanes.sanitized(tmp_path, "global_on_host.cpp", "GLOBAL_ON_HOST_MAIN", 23, 2, 3, 15, 16, 17, 33, 120, 6, 6, 6, 6, 6, 6, 6, 6)
    ra = [ln for ln in stdout.split("\n") if ln.startswith("rotation averaging")][0].split()
    assert 20 < int(ra[5]) <= 40 and float(ra[8]) < 0.05
    gp = [ln for ln in stdout.split("\n") if ln.startswith("global positioning")][0].split()
    assert gp[3] == "0" and gp[5] == "8" and int(gp[9]) >= 10 and 5.0 < float(gp[-1]) < 40.0
