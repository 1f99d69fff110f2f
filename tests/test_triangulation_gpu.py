"""Track triangulation on the GPU (csrc/pxr_triangulate.hip) against the numpy reference of tests/triangulation_cases.py,
and the inverse camera model against the oracle's forward model.

State: written together with the kernels and held to the same reference as tests/test_triangulation_lanes_cpu.py (the kernels'
source run lane by lane on the CPU, which passes); the first run on an MI355X is still to come."""
import functools

import numpy as np
import pytest

import pxo
import triangulation_cases as tc

pytestmark = pytest.mark.gpu

# lane-group boundaries (15, 16, 17), the LDS staging limit (33 > 32), the hypothesis cap (23: P = 253 <= 256; 24: P = 276, the first
# subsampled length), several 16-ray chunks (64, 65, 97; 97 > 96 cameras: one image seen twice), the degenerate 0 and 1
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 23, 24, 33, 64, 65, 97)
EXCUSE_MARGIN = 1e-9       # a track may differ from the reference only where the reference itself sits this close to a threshold


@functools.lru_cache(maxsize=None)
def _scene(kind):
    if kind == "boundaries":
        lengths = np.repeat(LENGTHS, 23)                               # 299 tracks: not a multiple of 4
        lengths = lengths[np.random.default_rng(1).permutation(len(lengths))]
        scene = tc.make_scene(lengths, n_cams=96, models=(2,), seed=3)
    else:                                                              # a pinhole, a radial and a fisheye camera in one call
        lengths = np.random.default_rng(2).integers(2, 12, 90)
        scene = tc.make_scene(lengths, n_cams=24, models=(1, 3, 5), seed=4, arc=9)
    return scene, tc.reference(scene)


def _run(ctx, scene, xyz=None, **options):
    from pixsfm_amd.engine import TriangulationProblem
    out = TriangulationProblem(ctx, scene).triangulate(xyz=xyz, **options)
    return dict(zip(("xyz", "status", "n_inliers", "obs_inlier", "obs_err"), (a.download() for a in out)))


def _compare(got, ref, scene):
    off = scene["track_offsets"]
    excused = ref["margin"] < EXCUSE_MARGIN
    print("tracks %d, status counts %s, smallest margin of the reference %.3g, excused %d" %
          (len(excused), np.bincount(ref["status"], minlength=4).tolist(), ref["margin"].min(), excused.sum()))
    assert excused.sum() <= 0.01 * len(excused)
    keep_t = ~excused
    keep_o = np.repeat(keep_t, np.diff(off))
    assert np.array_equal(got["status"][keep_t], ref["status"][keep_t])
    assert np.array_equal(got["n_inliers"][keep_t], ref["n_inliers"][keep_t])
    assert np.array_equal(got["obs_inlier"][keep_o], ref["obs_inlier"][keep_o])
    ok = keep_t & (ref["status"] == 0)
    dx = np.abs(got["xyz"][ok] - ref["xyz"][ok]).max()
    have = ~np.isnan(ref["obs_err"]) & keep_o
    assert np.array_equal(np.isnan(got["obs_err"][keep_o]), np.isnan(ref["obs_err"][keep_o]))
    de = np.abs(got["obs_err"][have] - ref["obs_err"][have]).max()
    print("max |xyz - reference| = %.3g, max |reproj_err - reference| = %.3g px over %d points" % (dx, de, ok.sum()))
    assert dx <= 1e-9 and de <= 1e-7
    assert np.isnan(got["xyz"][keep_t & (ref["status"] != 0)]).all()          # _run's sentinel


def test_image_to_world_inverts_all_models(ctx):
    from pixsfm_amd.engine import image_to_world
    grid = tc.polar_grid()                                       # 13 radii 0 .. 1 x 8 angles
    models = sorted(tc.MODEL_PARAMS)
    uv0 = np.tile(grid, (len(models), 1))
    cam = np.repeat(np.arange(len(models), dtype=np.int32), len(grid))
    xy = np.array([pxo.world_to_image(models[c], np.array(tc.MODEL_PARAMS[models[c]]), u, v)[0] for c, (u, v) in zip(cam, uv0)])
    assert len(xy) % 64 != 0
    uv, ok = image_to_world(ctx, models, tc.pad_params([tc.MODEL_PARAMS[m] for m in models]), xy, cam)
    err = np.abs(uv - uv0).max(axis=1)
    for c, m in enumerate(models):
        print("model %2d: max |uv - uv0| = %.3g" % (m, err[cam == c].max()))
    assert ok.all() and err.max() <= 1e-12
    # a pixel that cannot be undistorted is flagged and leaves its neighbours alone
    bad = xy.copy()
    rows = [70, 300, len(xy) - 1]                                 # SIMPLE_PINHOLE (closed form), SIMPLE_RADIAL (Newton), THIN_PRISM_FISHEYE
    bad[rows[0], 0] = np.nan; bad[rows[1], 1] = np.nan; bad[rows[2]] = np.inf
    uv_b, ok_b = image_to_world(ctx, models, tc.pad_params([tc.MODEL_PARAMS[m] for m in models]), bad, cam)
    assert not ok_b[rows].any() and np.isnan(uv_b[rows]).all()
    rest = np.setdiff1d(np.arange(len(xy)), rows)
    assert ok_b[rest].all() and np.array_equal(uv_b[rest], uv[rest])
    # one camera, no index array
    m = 4
    sel = cam == models.index(m)
    uv1, ok1 = image_to_world(ctx, [m], [tc.MODEL_PARAMS[m]], xy[sel])
    assert ok1.all() and np.array_equal(uv1, uv[sel])


def test_kernel_matches_the_reference_at_group_and_cap_boundaries(ctx):
    scene, ref = _scene("boundaries")
    assert len(scene["track_offsets"]) - 1 == 299 and (ref["margin"] >= EXCUSE_MARGIN).all()      # this generator excuses none
    assert set(np.diff(scene["track_offsets"])) == set(LENGTHS)
    assert {0, 1}.issubset(set(ref["status"]))
    _compare(_run(ctx, scene), ref, scene)


def test_every_status_code_and_the_sentinel(ctx):
    scene = tc.status_scene()
    ref = tc.reference(scene)
    assert ref["status"].tolist() == [1, 2, 3]
    sentinel = np.arange(9.0).reshape(3, 3) - 100
    got = _run(ctx, scene, xyz=sentinel)
    assert got["status"].tolist() == [1, 2, 3] and got["n_inliers"].tolist() == [0, 0, 0]
    assert np.array_equal(got["xyz"], sentinel)
    assert not got["obs_inlier"].any() and np.isnan(got["obs_err"]).all()
    # and the accepted track next to them keeps its neighbours' rows
    scene2, ref2 = _scene("mixed")
    s2 = np.full((len(ref2["status"]), 3), -7.0)
    got2 = _run(ctx, scene2, xyz=s2)
    assert (got2["xyz"][ref2["status"] != 0] == -7.0).all() and (ref2["status"] == 0).any()


def test_mixed_camera_models_in_one_call(ctx):
    scene, ref = _scene("mixed")
    assert set(scene["cam_model"]) == {1, 3, 5} and (ref["margin"] >= EXCUSE_MARGIN).all()
    _compare(_run(ctx, scene), ref, scene)


def test_unusable_observations_are_left_out(ctx):
    """A NaN keypoint cannot be undistorted: its track goes on without it (the reference drops it the same way)."""
    scene, _ = _scene("mixed")
    scene = dict(scene, obs_xy=scene["obs_xy"].copy())
    off = scene["track_offsets"]
    long_tracks = np.flatnonzero(np.diff(off) >= 5)[:6]
    for k, t in enumerate(long_tracks):
        scene["obs_xy"][off[t] + (k % 5)] = np.nan
    scene["obs_xy"][off[np.flatnonzero(np.diff(off) == 2)[0]]] = np.nan            # a 2-view track drops to one: status 1
    ref = tc.reference(scene)
    assert (ref["margin"] >= EXCUSE_MARGIN).all() and (ref["status"] == 1).any()
    _compare(_run(ctx, scene), ref, scene)


def test_repeatable_and_independent_of_track_order(ctx):
    scene, _ = _scene("boundaries")
    a, b = _run(ctx, scene), _run(ctx, scene)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    off = scene["track_offsets"]
    T = len(off) - 1
    perm = np.random.default_rng(9).permutation(T)
    lens = np.diff(off)
    new_off = np.concatenate([[0], np.cumsum(lens[perm])])
    obs = np.concatenate([np.arange(off[t], off[t + 1]) for t in perm])
    shuffled = dict(scene, track_offsets=new_off, obs_image=scene["obs_image"][obs], obs_xy=scene["obs_xy"][obs])
    c = _run(ctx, shuffled)
    for k in ("xyz", "status", "n_inliers"):
        assert np.array_equal(c[k], a[k][perm], equal_nan=True), k
    for k in ("obs_inlier", "obs_err"):
        assert np.array_equal(c[k], a[k][obs], equal_nan=True), k


def test_invalid_offsets_and_image_indices_are_refused(ctx):
    from pixsfm_amd import PixsfmHipError
    from pixsfm_amd._lib import load
    from pixsfm_amd.engine import TriangulationProblem
    scene = tc.status_scene()
    cases = {"not monotone": dict(track_offsets=np.array([0, 3, 1, 6], np.int64)),
             "n_obs": dict(track_offsets=np.array([0, 1, 3, 5], np.int64)),
             "negative": dict(track_offsets=np.array([-1, 1, 3, 6], np.int64)),
             "image": dict(obs_image=np.array([0, 0, 1, 0, 3, 2], np.int32)),
             "image ": dict(obs_image=np.array([0, -1, 1, 0, 1, 2], np.int32)),
             "camera": dict(image_camera=np.array([0, 1, 0], np.int32))}
    for what, change in cases.items():
        prob = TriangulationProblem(ctx, dict(scene, **change))
        with pytest.raises(PixsfmHipError) as e:
            prob.triangulate()
        assert e.value.code == -1, what                                          # PXR_EINVAL
        msg = load().pxr_last_error().decode()
        assert "pxr_triangulate_tracks" in msg and what.strip().split()[-1] in msg, (what, msg)
    # the context is as usable as before
    assert _run(ctx, scene)["status"].tolist() == [1, 2, 3]


def _api_scene():
    """A Graph over 10 images x 30 keypoints from synthetic matches (two of them wrong), noisy keypoints, posed images."""
    from pixsfm_amd.api import base
    from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction
    rng = np.random.default_rng(21)
    n_img, n_pts = 10, 30
    scene = tc.make_scene([n_img] * n_pts, n_cams=n_img, models=(2, 4), seed=22, p_outlier=0.0, arc=n_img)
    rec = Reconstruction()
    for c, m in enumerate((2, 4)):
        rec.add_camera(Camera(c + 1, m, 1000, 960, tc.MODEL_PARAMS[m]))
    names = ["im%02d.jpg" % i for i in range(n_img)]
    for i in range(n_img):
        rec.add_image(Image(i + 1, names[i], int(scene["image_camera"][i]) + 1, scene["qvec"][i], scene["tvec"][i]))
    # keypoint p of image i is the observation of point p in image i (make_scene permutes the cameras inside a track)
    keypoints = {n: np.zeros((n_pts, 2)) for n in names}
    off = scene["track_offsets"]
    for p in range(n_pts):
        for o in range(off[p], off[p + 1]):
            keypoints[names[scene["obs_image"][o]]][p] = scene["obs_xy"][o]
    g = base.Graph()
    for i in range(n_img):
        for j in (i + 1, i + 2):
            if j < n_img:
                m = np.stack([np.arange(n_pts), np.arange(n_pts)], 1)
                g.register_matches(names[i], names[j], m, rng.uniform(0.5, 1.0, n_pts))
    g.register_matches(names[0], names[5], [[3, 17]], [0.05])            # two wrong matches (weak: the labelling keeps the tracks apart)
    g.register_matches(names[2], names[7], [[11, 4]], [0.05])
    return rec, keypoints, g, scene


def test_api_end_to_end(ctx):
    from pixsfm_amd.api import BundleAdjuster, TrackTriangulator, base
    from pixsfm_amd.api.triangulation import flatten_tracks
    rec, keypoints, g, scene = _api_scene()
    labels = base.compute_track_labels(g)
    q0 = {i: im.qvec.copy() for i, im in rec.images.items()}
    t0 = {i: im.tvec.copy() for i, im in rec.images.items()}
    k0 = {c: cam.params.copy() for c, cam in rec.cameras.items()}

    plain = TrackTriangulator.create({"refine": False}, ctx=ctx)
    out, summary = plain.triangulate(rec, keypoints, g, track_labels=labels)
    flat = flatten_tracks(rec, keypoints, g, labels)
    direct = _run(ctx, flat)
    ref = tc.reference(flat)
    _compare(direct, ref, flat)
    assert summary["num_tracks"] == len(flat["track_label"]) == 30 and summary["num_points3D"] == (direct["status"] == 0).sum() == 30
    assert summary["status"]["ok"] == 30 and summary["mean_track_length"] == direct["n_inliers"].mean()
    assert out is not rec and not rec.points3D and len(out.points3D) == 30
    for t, pid in plain.last["point3D_of_track"].items():
        assert np.array_equal(out.points3D[pid].xyz, direct["xyz"][t])
        assert out.points3D[pid].track.length() == direct["n_inliers"][t]
    assert all(len(out.images[i].points2D) == 30 for i in out.images)
    # labels from the graph (device labelling with a context) give the same model
    out_b, _ = plain.triangulate(rec, keypoints, g)
    assert all(np.array_equal(out_b.points3D[p].xyz, out.points3D[p].xyz) for p in out.points3D)

    refined, summary_r = TrackTriangulator.create({}, ctx=ctx).triangulate(rec, keypoints, g, track_labels=labels)
    print("mean reprojection error %.4f px -> %.4f px after the points-only refinement" %
          (summary_r["mean_reprojection_error"], summary_r["mean_reprojection_error_refined"]))
    assert summary_r["mean_reprojection_error"] == summary["mean_reprojection_error"]
    assert summary_r["mean_reprojection_error_refined"] <= summary_r["mean_reprojection_error"]
    for r in (rec, refined):
        for i, im in r.images.items():
            assert np.array_equal(im.qvec, q0[i]) and np.array_equal(im.tvec, t0[i])
        for c, cam in r.cameras.items():
            assert np.array_equal(cam.params, k0[c])
    moved = max(np.abs(refined.points3D[p].xyz - out.points3D[p].xyz).max() for p in out.points3D)
    assert 0 < moved < 0.05
    point_of_track = flat["obs_feature"][flat["track_offsets"][:-1]]               # keypoint p of every image observes point p
    err_before = np.median([np.linalg.norm(out.points3D[p].xyz - scene["gt_xyz"][point_of_track[t]])
                            for t, p in plain.last["point3D_of_track"].items()])
    assert err_before < 0.02
    # ... and the model goes straight into the geometric bundle adjustment
    res = BundleAdjuster.create({"strategy": "geometric"}).refine(refined)
    assert res["summary"] is not None
