"""The host side of incremental mapping without a GPU: the numpy reference of pxr_mapper_visibility on answers worked out by hand,
the flat-array helpers of engine.MapperScene against Python loops, the mapper's initial-pair order, gauge and configuration, and
what the trap scenes of tests/test_mapping_gpu.py promise."""
import numpy as np
import pytest

import mapping_cases as mc


def _one_image(xy, size=(640, 480), status=None, xyz=None):
    n = len(xy)
    scene = dict(track_offsets=np.arange(n + 1), obs_image=np.zeros(n, np.int32), obs_xy=np.array(xy, dtype=np.float64).reshape(-1, 2),
                 image_camera=np.zeros(1, np.int32), cam_model=np.array([0], np.int32), cam_size=np.array([size], np.int32))
    return scene, (np.zeros((n, 3)) if xyz is None else xyz), (np.zeros(n, np.int32) if status is None else status)


@pytest.mark.parametrize("levels", [1, 3, 6])
def test_reference_on_known_answers(levels):
    full = sum(4 ** l for l in range(1, levels + 1))
    scene, xyz, status = _one_image([[100.0, 100.0]])
    ref = mc.visibility_reference(scene, xyz, status, [1], levels)
    assert ref["n_visible"].tolist() == [1] and ref["score"].tolist() == [full]                 # one point: 4 + 16 + ... + 4^L
    scene, xyz, status = _one_image([[100.0, 100.0], [100.5, 100.5], [630.0, 470.0]])
    ref = mc.visibility_reference(scene, xyz, status, [1], levels)
    assert ref["n_visible"].tolist() == [3] and ref["score"].tolist() == [2 * full]             # two share the finest cell; opposite corners
    assert ref["corr_offsets"].tolist() == [0, 3] and ref["corr_obs"].tolist() == [0, 1, 2]
    # the four quadrants: all of level 1, four distinct cells at every level
    scene, xyz, status = _one_image([[1.0, 1.0], [639.0, 1.0], [1.0, 479.0], [639.0, 479.0]])
    assert mc.visibility_reference(scene, xyz, status, [1], levels)["score"].tolist() == [4 * full]
    # outside the image the cells clamp: (-50, -50) falls into the cell of (0, 0), (700, 500) into that of the far corner
    scene, xyz, status = _one_image([[-50.0, -50.0], [0.0, 0.0], [700.0, 500.0], [639.9, 479.9], [640.0, 480.0]])
    assert mc.visibility_reference(scene, xyz, status, [1], levels)["score"].tolist() == [2 * full]
    # masked out; a track without a point; a point or a keypoint that is not finite
    assert mc.visibility_reference(scene, xyz, status, [0], levels)["score"].tolist() == [0]
    scene, xyz, status = _one_image([[10.0, 10.0], [300.0, 200.0], [np.nan, 5.0], [600.0, 400.0]], status=np.array([0, 2, 0, 0], np.int32),
                                    xyz=np.array([[0, 0, 1.0], [0, 0, 1.0], [0, 0, 1.0], [0, np.inf, 1.0]]))
    ref = mc.visibility_reference(scene, xyz, status, [1], levels)
    assert ref["n_visible"].tolist() == [1] and ref["corr_obs"].tolist() == [0] and ref["n_corr"] == 1


def test_cell_borders():
    assert mc.cell(0.0, 6, 640) == 0 and mc.cell(9.999, 6, 640) == 0 and mc.cell(10.0, 6, 640) == 1      # 640 / 64 = 10 px per cell
    assert mc.cell(639.999, 6, 640) == 63 and mc.cell(640.0, 6, 640) == 63 and mc.cell(1e300, 6, 640) == 63
    assert mc.cell(-1e300, 6, 640) == 0 and mc.cell(320.0, 1, 640) == 1 and mc.cell(319.999, 1, 640) == 0


def test_boundary_batch_is_what_it_says():
    scene, xyz, status, mask, planned = mc.boundary_batch()
    assert len(mask) == 11 and planned.tolist()[:9] == list(mc.VISIBLE_COUNTS)
    ref = mc.visibility_reference(scene, xyz, status, mask, 6)
    assert ref["n_visible"].tolist() == planned.tolist()
    assert ref["score"][9] == 0 and ref["score"][10] == 0 and ref["score"][0] == 0 and (ref["score"][1:9] > 0).all()
    assert len(set(scene["cam_size"][scene["image_camera"]][:, 0])) == 2
    xy = scene["obs_xy"]
    assert np.isnan(xy).any() and np.isinf(xy).any() and (xy[np.isfinite(xy)] < 0).any() and (xy[np.isfinite(xy)] > 1000).any()
    obs_track = np.repeat(np.arange(len(status)), np.diff(scene["track_offsets"]))
    in4 = obs_track[scene["obs_image"] == 4]
    assert len(np.unique(in4)) < len(in4)                                                          # a track seen twice by one image


def test_transpose_and_restricted_tracks_against_loops():
    from pixsfm_amd.engine import MapperScene, image_major_transpose, restrict_tracks
    scene = mc.boundary_batch()[0]
    obs_image, off = scene["obs_image"], scene["track_offsets"]
    n_images = len(scene["image_camera"])
    io, iobs = image_major_transpose(obs_image, n_images)
    want = [[o for o in range(len(obs_image)) if obs_image[o] == i] for i in range(n_images)]
    assert io.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert iobs.tolist() == [o for w in want for o in w] and iobs.dtype == np.int64 and io.dtype == np.int64
    with pytest.raises(ValueError):
        image_major_transpose([0, 3], 3)
    registered = np.zeros(n_images, bool)
    registered[[2, 5, 8]] = True
    r_off, r_idx = restrict_tracks(off, obs_image, registered)
    keep, loop_off = [], [0]
    for t in range(len(off) - 1):
        keep += [o for o in range(off[t], off[t + 1]) if registered[obs_image[o]]]
        loop_off.append(len(keep))
    assert r_off.tolist() == loop_off and r_idx.tolist() == keep and len(r_off) == len(off)       # the track count is unchanged
    s = MapperScene(None, scene)
    r = s.restricted_tracks(registered)
    assert r["track_offsets"].tolist() == loop_off and np.array_equal(r["obs_image"], obs_image[keep])
    assert np.array_equal(r["obs_xy"], scene["obs_xy"][keep], equal_nan=True)
    assert s.obs_track.tolist() == np.repeat(np.arange(len(off) - 1), np.diff(off)).tolist()
    none = s.restricted_tracks(np.zeros(n_images, bool))
    assert none["track_offsets"].tolist() == [0] * len(off) and len(none["obs_index"]) == 0


def test_initial_pair_order_and_gauge():
    from pixsfm_amd.api.mapping import gauge_component, initial_pair_order, median_triangulation_angle
    g = [dict(success=True, num_inliers=50), dict(success=False), dict(success=True, num_inliers=80, config="PANORAMIC"),
         dict(success=True, num_inliers=80, config="PLANAR"), dict(success=True, num_inliers=80), dict(success=True, num_inliers=120, config="CALIBRATED"),
         dict(success=True, num_inliers=200, config="DEGENERATE")]
    assert initial_pair_order(g, 20) == [5, 3, 4, 0]                       # inliers descending, pair index ascending
    assert initial_pair_order(g, 2) == [5, 3] and initial_pair_order(g, 0) == []
    assert gauge_component([0.1, -0.9, 0.3]) == 1 and gauge_component([0.5, 0.2, -0.5]) == 0 and gauge_component([0, 0, 1e-9]) == 2
    X = np.array([[0.0, 0.0, 1.0]])
    assert abs(median_triangulation_angle(X, np.array([-1.0, 0, 0]), np.array([1.0, 0, 0])) - 90.0) < 1e-9
    assert median_triangulation_angle(np.empty((0, 3)), np.zeros(3), np.ones(3)) == 0.0


def test_conf_validation_and_defaults():
    from pixsfm_amd.api import IncrementalMapper, TrackTriangulator
    d = IncrementalMapper.default_conf
    assert (d['init_min_num_inliers'], d['init_min_tri_angle'], d['init_max_trials']) == (100, 16.0, 20)
    assert (d['abs_pose_max_error'], d['abs_pose_min_num_inliers'], d['abs_pose_min_inlier_ratio']) == (12.0, 30, 0.25)
    assert (d['max_reg_trials'], d['max_images_per_round'], d['pyramid_levels']) == (3, 0, 6)
    assert (d['filter_max_reproj_error'], d['ba_max_num_iterations'], d['ba_refine_focal_length']) == (4.0, 50, False)
    assert d['triangulation'] == {k: v for k, v in TrackTriangulator.default_conf.items() if k != 'refine'}
    assert IncrementalMapper.create({'max_images_per_round': 1, 'triangulation': {'min_tri_angle': 2.0}}).conf['triangulation']['max_hypotheses'] == 256
    for bad in ({'pyramid_levels': 0}, {'pyramid_levels': 7}, {'no_such_key': 1}, {'max_images_per_round': -1}, {'max_reg_trials': 0},
                {'abs_pose_min_inlier_ratio': 1.5}, {'abs_pose_max_error': 0.0}, {'triangulation': {'refine': True}},
                {'init_min_tri_angle': 180.0}):
        with pytest.raises(ValueError):
            IncrementalMapper.create(bad)


def test_the_library_exports_the_entry_points():
    from pixsfm_amd import _lib
    lib = _lib.load()
    assert {"pxr_mapper_visibility", "pxr_mapper_visibility_timed"} <= set(_lib.declared_symbols())
    assert lib.pxr_mapper_visibility and lib.pxr_mapper_visibility_timed


def test_trap_scenes_hold_their_traps():
    # the co-centred image and image 0 share the most matches of all pairs
    s = mc.ring_scene(cocentred=True, seed=0)
    pairs, matches = mc.matches_from_labels(s)
    most = max(range(len(pairs)), key=lambda p: len(matches[p]))
    assert set(pairs[most]) == {s["names"][0], s["names"][-1]}
    c = [-mc.synthetic.qvec_to_rotmat(q).T @ t for q, t in (s["poses"][s["names"][0]], s["poses"][s["names"][-1]])]
    assert np.linalg.norm(c[0] - c[1]) < 1e-12
    # a second component shares no match with the first; an unmatched image is in no pair
    s = mc.ring_scene(n_images_second=4, unmatched=1, seed=0)
    pairs, _ = mc.matches_from_labels(s)
    first, second = set(s["names"][:10]), set(s["names"][10:14])
    assert all(({a, b} <= first) or ({a, b} <= second) for a, b in pairs) and any({a, b} <= second for a, b in pairs)
    # a tenth of the members sits in a wrong track
    s = mc.ring_scene(wrong_share=0.1, seed=mc.WRONG_SEED)
    n_wrong, n_all = sum(w.sum() for w in s["wrong"].values()), sum(len(w) for w in s["wrong"].values())
    assert 0.07 * n_all < n_wrong < 0.13 * n_all
    assert mc.wrong_member_clearance(s) > 12.0                             # no wrong member that geometry could not tell from a right one
    assert all((s["label_of"][n][s["wrong"][n]] != s["owner"][n][s["wrong"][n]]).all() for n in s["names"])


def test_umeyama_recovers_a_similarity():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((20, 3))
    R = mc.synthetic.qvec_to_rotmat(np.array([0.9, 0.1, -0.3, 0.2]))
    s, R2, t = mc.umeyama(A, 2.5 * A @ R.T + [1.0, -2.0, 3.0])
    assert abs(s - 2.5) < 1e-12 and np.abs(R2 - R).max() < 1e-12 and np.abs(t - [1.0, -2.0, 3.0]).max() < 1e-12
