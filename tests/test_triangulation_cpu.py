"""Track triangulation without a GPU: the numpy reference of the estimator (tests/triangulation_cases.py) is pinned against
linear algebra and against ground truth, the undistortion the kernel restates converges as DESIGN.md section 18 says, and
the host logic of pixsfm_amd.api.triangulation (flattening, defaults, struct layouts) is checked."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pxo
import triangulation_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_is_the_least_squares_point_to_the_rays():
    rng = np.random.default_rng(0)
    for n in (2, 3, 7, 40):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        c = rng.normal(size=(n, 3)) * 5
        M = np.concatenate([np.eye(3) - np.outer(x, x) for x in d])            # stacked projectors
        rhs = np.concatenate([(np.eye(3) - np.outer(x, x)) @ y for x, y in zip(d, c)])
        want = np.linalg.lstsq(M, rhs, rcond=None)[0]
        got = tc.solve(d, c, range(n))
        assert np.abs(got - want).max() < 1e-11 * max(1.0, np.abs(want).max())
    # two rays: the midpoint of their common perpendicular
    d = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    c = np.array([[0.0, 0, 0], [0, 0, 2.0]])
    assert np.allclose(tc.solve(d, c, (0, 1)), [0, 0, 1.0], atol=1e-15)


def test_oracle_newton_undistortion_converges_in_five_steps():
    worst, steps = 0.0, 0
    for model, k in tc.MODEL_PARAMS.items():
        for u, v in tc.polar_grid():
            xy = pxo.world_to_image(model, np.array(k), u, v)[0]
            uu, vv, ok, it = tc.image_to_world(model, k, *xy)
            assert ok, (model, u, v)
            worst, steps = max(worst, abs(uu - u), abs(vv - v)), max(steps, it)
    print("undistortion: worst |uv - uv0| = %.3g after at most %d steps" % (worst, steps))
    assert steps <= 5 and worst < 6e-16
    assert not tc.image_to_world(2, tc.MODEL_PARAMS[2], np.nan, 3.0)[2]


def test_reference_recovers_the_true_inliers():
    """1 500 tracks of 2-8 views over 12 cameras, sigma 0.5 px, 20 % outliers in tracks of >= 4 views."""
    lengths = np.random.default_rng(5).integers(2, 9, 1500)
    scene = tc.make_scene(lengths, n_cams=12, seed=11, arc=5)
    ref = tc.reference(scene)
    off = scene["track_offsets"]
    good = total = 0
    errs = []
    for t in range(len(lengths)):
        truth = scene["true_inlier"][off[t]:off[t + 1]]
        if truth.sum() < 2:
            continue
        total += 1
        if ref["status"][t] == 0 and np.array_equal(ref["obs_inlier"][off[t]:off[t + 1]].astype(bool), truth):
            good += 1
            errs.append(np.linalg.norm(ref["xyz"][t] - scene["gt_xyz"][t]))
            assert ref["n_inliers"][t] == truth.sum()
            assert np.nanmax(ref["obs_err"][off[t]:off[t + 1]][truth]) <= 4.0
    print("true inlier set recovered on %d of %d tracks, median point error %.4f" % (good, total, np.median(errs)))
    assert good >= 0.99 * total
    assert np.median(errs) < 0.02          # the points fill [-1, 1]^3 at distance 10: 0.5 px at f = 1200 is 4e-3 there


def test_hypothesis_subsampling_rule():
    assert np.array_equal(tc.hypothesis_pairs(23, 256), np.arange(253))           # P = 253 <= 256: all pairs
    for n in (24, 33, 97):
        P = n * (n - 1) // 2
        idx = tc.hypothesis_pairs(n, 256)
        assert len(idx) == 256 and idx[0] == 0 and np.all(np.diff(idx) > 0) and idx[-1] < P
        a, b = tc._pairs(n)
        assert (a[idx[0]], b[idx[0]]) == (0, 1)
        assert np.array_equal(idx, [h * P // 256 for h in range(256)])


def _graph_scene():
    from pixsfm_amd.api import base
    from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction
    rec = Reconstruction()
    rec.add_camera(Camera(7, "SIMPLE_RADIAL", 1000, 960, tc.MODEL_PARAMS[2]))
    rec.add_camera(Camera(3, "PINHOLE", 1000, 960, tc.MODEL_PARAMS[1]))
    for image_id, name, cam in ((5, "b.jpg", 7), (2, "a.jpg", 3), (9, "c.jpg", 7)):
        q, t = tc.look_at_pose([10.0, 0.0, float(image_id)])
        rec.add_image(Image(image_id, name, cam, q, t))
    g = base.Graph()
    g.register_matches("a.jpg", "b.jpg", [[0, 1], [2, 0]], [0.9, 0.8])
    g.register_matches("b.jpg", "x.jpg", [[1, 4]], [0.7])                          # x.jpg is not in the reconstruction
    g.register_matches("b.jpg", "c.jpg", [[1, 3], [2, 2]], [0.6, 0.5])
    keypoints = {n: np.arange(10.0).reshape(5, 2) + 100 * i for i, n in enumerate(("a.jpg", "b.jpg", "c.jpg", "x.jpg"))}
    return rec, g, keypoints


def test_flattening_drops_foreign_images_and_unlabelled_nodes():
    from pixsfm_amd.api.triangulation import flatten_tracks
    rec, g, keypoints = _graph_scene()
    # nodes in creation order: a0 b1 a2 b0 x4 c3 b2 c2
    assert [(n.image_id, n.feature_idx) for n in g.nodes] == [(0, 0), (1, 1), (0, 2), (1, 0), (2, 4), (3, 3), (1, 2), (3, 2)]
    labels = [4, 4, 1, 1, 4, 4, -1, 0]
    flat = flatten_tracks(rec, keypoints, g, labels)
    assert flat["image_ids"] == [2, 5, 9] and flat["camera_ids"] == [3, 7]
    assert flat["image_camera"].tolist() == [0, 1, 1] and flat["cam_model"].tolist() == [1, 2]
    assert flat["cam_params"].shape == (2, 12) and flat["cam_params"][1, :4].tolist() == tc.MODEL_PARAMS[2]
    assert flat["track_label"].tolist() == [0, 1, 4]
    assert flat["track_offsets"].tolist() == [0, 1, 3, 6] and flat["track_offsets"].dtype == np.int64
    # label 0: c2; label 1: a2 b0; label 4: a0 b1 (x4 dropped) c3; b2 (label -1) dropped
    assert flat["obs_image"].tolist() == [2, 0, 1, 0, 1, 2] and flat["obs_image"].dtype == np.int32
    assert flat["obs_feature"].tolist() == [2, 2, 0, 0, 1, 3]
    want = [keypoints["c.jpg"][2], keypoints["a.jpg"][2], keypoints["b.jpg"][0], keypoints["a.jpg"][0], keypoints["b.jpg"][1],
            keypoints["c.jpg"][3]]
    assert np.array_equal(flat["obs_xy"], want)
    assert np.array_equal(flat["qvec"][1], rec.images[5].qvec) and np.array_equal(flat["tvec"][2], rec.images[9].tvec)
    with pytest.raises(ValueError):
        flatten_tracks(rec, keypoints, g, labels[:-1])


def test_build_reconstruction_keeps_all_keypoints_and_only_inlier_tracks():
    from pixsfm_amd.api.triangulation import build_reconstruction, flatten_tracks
    rec, g, keypoints = _graph_scene()
    flat = flatten_tracks(rec, keypoints, g, [4, 4, 1, 1, 4, 4, -1, 0])
    xyz = np.array([[0.0, 0, 0], [1.0, 2, 3], [4.0, 5, 6]])
    out, of_track = build_reconstruction(rec, keypoints, flat, xyz, np.array([1, 0, 0]), np.array([0, 1, 1, 1, 0, 1], np.uint8))
    assert out is not rec and sorted(out.images) == [2, 5, 9] and sorted(out.cameras) == [3, 7]
    assert [len(out.images[i].points2D) for i in (2, 5, 9)] == [5, 5, 5]
    assert of_track == {1: 1, 2: 2} and out.point3D_ids() == [1, 2]
    assert [(e.image_id, e.point2D_idx) for e in out.points3D[1].track.elements] == [(2, 2), (5, 0)]
    assert [(e.image_id, e.point2D_idx) for e in out.points3D[2].track.elements] == [(2, 0), (9, 3)]       # b1 is no inlier
    assert out.images[2].points2D[2].point3D_id == 1 and out.images[9].points2D[3].point3D_id == 2
    assert not out.images[5].points2D[1].has_point3D() and np.array_equal(out.points3D[2].xyz, [4.0, 5, 6])
    assert out.num_observations() == 4 and not rec.points3D


def test_default_conf_and_options():
    from pixsfm_amd.api import TrackTriangulator
    from pixsfm_amd.engine import tri_options
    assert TrackTriangulator.default_conf == {'min_tri_angle': 1.5, 'max_angle_error': 2.0, 'max_reproj_error': 4.0,
                                              'min_track_len': 2, 'max_hypotheses': 256, 'refine': True}
    t = TrackTriangulator.create({'refine': False, 'max_hypotheses': 64})
    assert t.conf['refine'] is False and t.options()['max_hypotheses'] == 64 and 'refine' not in t.options()
    with pytest.raises(ValueError):
        TrackTriangulator.create({'ransac': True})
    o = tri_options()
    assert (o.min_tri_angle, o.max_angle_error, o.max_reproj_error, o.min_track_len, o.max_hypotheses) == (1.5, 2.0, 4.0, 2, 256)
    assert tc.DEFAULTS == TrackTriangulator.create({}).options()


def test_triangulation_struct_layouts_match_the_c_compiler(tmp_path):
    from pixsfm_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = {"pxr_tri_view": _lib.TriView, "pxr_tri_options": _lib.TriOptions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pixsfm_hip.h"', 'int main(void) {']
    for cname, ct in structs.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        cname, field, val = ln.split()
        ct = structs[cname]
        want = ctypes.sizeof(ct) if field == "sizeof" else getattr(ct, field).offset
        assert int(val) == want, (cname, field, val, want)
        seen += 1
    assert seen == 2 + 12 + 5
    assert ctypes.sizeof(_lib.TriView) == 96 and ctypes.sizeof(_lib.TriOptions) == 32
