"""CPU: the numpy references of global mapping (tests/global_mapping_cases.py) against ground truth on the two scenes of the issue,
the pose conventions, the degenerate inputs, and the host logic of pixsfm_amd.api.global_mapping (view graph, components, conf)."""
import numpy as np
import pytest

import global_mapping_cases as gc


# ---- the reference against ground truth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.SCENES))
def test_reference_recovers_the_corrupted_ring(name):
    """5 % of the observations and 10 % of the pairs are random.  Conditions: max rotation error <= 1 degree, max centre error
    <= 2 % of the ring radius; the figures recorded in the cases file (what the GPU tests are bounded against) still hold."""
    scene, ra, b, gp = gc.solved(name)
    rot = gc.rotation_errors_deg(ra["qvec"], scene["qvec_gt"], ra["root"]).max()
    aligned = gc.similarity_align(gp["centre"], scene["centre_gt"])[0]
    cen = np.linalg.norm(aligned - scene["centre_gt"], axis=1).max()
    print("%s: %d iterations, max rotation error %.4f deg, max centre error %.5f, %d rounds" % (name, ra["iterations"], rot, cen, gp["rounds"]))
    assert rot <= 1.0 and cen <= 0.02 * gc.RADIUS and gp["status"] == 0
    want = gc.REFERENCE_ERRORS[name]
    assert ra["iterations"] == want["iterations"]
    assert rot == pytest.approx(want["max_rotation_deg"], rel=1e-2) and cen == pytest.approx(want["max_centre"], rel=1e-2)
    # every random pair ends above GlobalMapper's default max_rotation_residual, and no other pair does
    assert np.array_equal(np.degrees(ra["pair_angle"]) > 10.0, scene["pair_is_outlier"])


# ---- conventions --------------------------------------------------------------------------------------------------------------------
def test_pair_conventions_are_the_two_view_verifiers():
    """TwoViewVerifier documents x2 = R x1 + t for a pair (image 1, image 2).  With image poses x_i = R_i X + t_i that is
    R_p = R_2 R_1^t and t = t_2 - R_p t_1, and the baseline direction b_p = -R_2^t t points from centre 1 to centre 2."""
    rng = np.random.default_rng(2)
    q = gc.qcanonical(rng.normal(size=(2, 4)))
    t = rng.normal(size=(2, 3))
    R = gc.qrot(q)
    c = -np.einsum("kji,kj->ki", R, t)
    Rp = R[1] @ R[0].T
    tp = t[1] - Rp @ t[0]
    X = rng.normal(size=3)
    assert np.allclose(R[1] @ X + t[1], Rp @ (R[0] @ X + t[0]) + tp)                    # x2 = R x1 + t
    qp = gc.rotmat_to_qvec(Rp)
    b = gc.pair_directions(q, [(0, 1)], tp[None])[0]
    assert np.allclose(b, (c[1] - c[0]) / np.linalg.norm(c[1] - c[0]))
    # the averaging puts image 2 at R_p R_1 in the frame of image 1 (root: equal weights, the first image)
    ra = gc.rotation_averaging_reference(2, [(0, 1)], qp[None], [1.0])
    assert ra["root"] == 0 and np.allclose(gc.qrot(ra["qvec"][1]), Rp) and ra["pair_angle"][0] < 1e-12
    # and the api's direction helper says the same
    from pixsfm_amd.api.global_mapping import baseline_directions
    assert np.allclose(baseline_directions(q, np.array([(0, 1)]), tp[None] / np.linalg.norm(tp))[0], b)


# ---- degeneracies -------------------------------------------------------------------------------------------------------------------
def test_parallel_rays_give_status_one_and_no_nan():
    """A track whose rays from three different images are parallel (the point at infinity) under the rotations in use."""
    scene = dict(gc.boundary_batch(22))
    q, t = scene["qvec_gt"], scene["tvec_gt"]
    direction = np.array([0.05, 0.02, -1.0]) / np.linalg.norm([0.05, 0.02, -1.0])
    r = np.einsum("kij,j->ki", gc.qrot(q[[0, 1, 2]]), direction)
    xy = np.stack([gc.FOCAL * r[:, 0] / r[:, 2] + gc.WIDTH / 2, gc.FOCAL * r[:, 1] / r[:, 2] + gc.HEIGHT / 2], axis=1)
    scene["track_offsets"] = np.concatenate([scene["track_offsets"], [scene["track_offsets"][-1] + 3]])
    scene["obs_image"] = np.concatenate([scene["obs_image"], [0, 1, 2]]).astype(np.int32)
    scene["obs_xy"] = np.concatenate([scene["obs_xy"], xy])
    b = gc.pair_directions(q, scene["pair_image"], scene["pair_tvec"])
    gp = gc.global_positioning_reference(scene, q, scene["pair_image"], b, scene["pair_weight"], 0)
    assert gp["status"] == 0 and gp["track_status"][-1] == 1 and (gp["obs_weight"][-3:] == 0).all()
    assert gp["track_status"][scene["special"]["parallel"]] == 1
    assert np.isfinite(gp["centre"]).all() and np.isfinite(gp["xyz"][gp["track_status"] == 0]).all()
    assert np.isfinite(gp["obs_weight"]).all() and np.isfinite(gp["pair_weight"]).all()


def test_an_image_without_observations_is_positioned_by_its_pairs():
    scene, ra, b, gp = gc.solved("boundary", 23)
    k = scene["special"]["empty_image"]
    assert not (scene["obs_image"] == k).any()
    aligned = gc.similarity_align(gp["centre"], scene["centre_gt"])[0]
    err = np.linalg.norm(aligned - scene["centre_gt"], axis=1)
    print("centre errors: empty image %.4f, largest %.4f" % (err[k], err.max()))
    # pairs alone: directions with 1 degree of noise per axis to neighbours 2.7 .. 8 away displace it by about 0.1; an image that was
    # not positioned would sit at the origin, 10 away
    assert err[k] <= 0.05 * gc.RADIUS


def test_two_components_are_refused_by_the_reference_and_unregistered_by_the_api():
    scene = gc.boundary_batch(22)
    half = gc.bad_rotation_inputs(scene)[-1][2]
    assert gc.rotation_averaging_reference(22, half, scene["pair_qvec"][:len(half)], scene["pair_weight"][:len(half)]) is None
    from pixsfm_amd.api.global_mapping import largest_component
    # images 0 .. 10 and 11 .. 21, eleven each: the tie goes to the component that holds the lowest image index
    assert largest_component(22, half).tolist() == [k <= 10 for k in range(22)]
    assert largest_component(22, half[:-1]).tolist() == [k <= 10 for k in range(22)]      # eleven against ten
    assert largest_component(22, half[1:]).tolist() == [k >= 11 for k in range(22)]       # ten (1 .. 10) against eleven
    assert largest_component(22, half, must_hold=15).tolist() == [k >= 11 for k in range(22)]


def _geometry(i, j, q, t, c, inliers=100, **extra):
    """The geometry of the pair (i, j) under ground truth (q, c)."""
    Rp = gc.qrot(q[j]) @ gc.qrot(q[i]).T
    base = (c[j] - c[i]) / np.linalg.norm(c[j] - c[i])
    return dict(success=True, qvec=gc.rotmat_to_qvec(Rp), tvec=-gc.qrot(q[j]) @ base, num_inliers=inliers, **extra)


def test_view_graph_selection():
    from pixsfm_amd.api.global_mapping import view_graph
    q, t, c = gc.ring_poses(6, np.random.default_rng(0))
    names = ["im%d" % k for k in range(6)]
    index = {nm: k for k, nm in enumerate(names)}
    pairs = [("im0", "im1"), ("im1", "im2"), ("im2", "im3"), ("im3", "im4"), ("im4", "im5"), ("im0", "nobody"), ("im2", "im2"),
             ("im3", "im5")]
    geoms = [_geometry(0, 1, q, t, c), _geometry(1, 2, q, t, c, config="PANORAMIC"), dict(success=False),
             _geometry(3, 4, q, t, c, config="UNCALIBRATED"), _geometry(4, 5, q, t, c, config="PLANAR", inliers=40),
             _geometry(0, 1, q, t, c), _geometry(2, 3, q, t, c), _geometry(3, 5, q, t, c, inliers=0)]      # no weight: joins nothing
    vg = view_graph(index, pairs, geoms)
    assert vg["index"].tolist() == [0, 1, 4] and vg["pair_image"].tolist() == [[0, 1], [1, 2], [4, 5]]
    assert vg["positional"].tolist() == [True, False, True] and vg["num_inliers"].tolist() == [100.0, 100.0, 40.0]
    assert np.allclose(np.linalg.norm(vg["pair_tvec"][[0, 2]], axis=1), 1.0) and (vg["pair_tvec"][1] == 0).all()


def test_pairs_above_the_residual_cut_images_off():
    """The logic GlobalMapper applies after the averaging, on a hand-made graph: a chain 0-1-2-3 plus a triangle edge 0-2; with the
    pair 2-3 removed image 3 is cut off, with 0-1 removed nothing is (1 stays joined through 1-2)."""
    from pixsfm_amd.api.global_mapping import largest_component
    pim = np.array([(0, 1), (1, 2), (2, 3), (0, 2)])
    assert largest_component(4, np.delete(pim, 2, axis=0), must_hold=0).tolist() == [True, True, True, False]
    assert largest_component(4, np.delete(pim, 0, axis=0), must_hold=0).all()
    assert largest_component(4, pim[:0], must_hold=2).tolist() == [False, False, True, False]


# ---- host logic of the api -----------------------------------------------------------------------------------------------------------
def test_conf_validation():
    from pixsfm_amd.api import GlobalMapper
    assert GlobalMapper.create({'positioning': {'iterations': 4}}).conf['positioning']['sigma_obs'] == 1.0
    for bad in ({'no_such_key': 1}, {'positioning': {'no_such_key': 1}}, {'max_rotation_residual': 0.0}, {'min_num_observations': -1},
                {'ba_max_num_iterations': 0}, {'filter_max_reproj_error': 0.0}, {'rotation_averaging': {'max_iterations': 0}}):
        with pytest.raises(ValueError):
            GlobalMapper.create(bad)


def test_positioning_graph_after_the_averaging():
    """GlobalMapper's chain after the averaging, on a hand-made view graph of six images: rows 0 .. 6 are the chain 0-1-2-3-4 with the
    triangle edge 0-2 and a PANORAMIC pair 1-3 (all averaged), row 7 joins image 5 to nobody averaged (another component)."""
    from pixsfm_amd.api.global_mapping import positioning_graph
    pim = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (1, 3), (5, 5)], np.int32)
    vg = dict(pair_image=pim, num_inliers=np.array([50.0, 60.0, 70.0, 80.0, 90.0, 40.0, 30.0, 10.0]),
              positional=np.array([True, True, True, True, True, False, True, True]), index=np.arange(8) + 100)
    use = np.array([True] * 7 + [False])
    # nothing above: every averaged pair takes part, the PANORAMIC one with weight 0; image 5 was never in
    pg = positioning_graph(vg, use, np.array([1.0, 2.0, 0.5, 3.0, 0.1, 4.0, 9.9]), 10.0, 2, 6)
    assert pg["above"].tolist() == [] and pg["rows"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert pg["comp"].tolist() == [True] * 5 + [False] and pg["weight"].tolist() == [50.0, 60.0, 70.0, 80.0, 90.0, 0.0, 30.0]
    # 2-3 and both 1-3 above: images 3 and 4 are cut off from the root 2, and the pair 3-4 leaves with them though its residual is small
    pg = positioning_graph(vg, use, np.array([1.0, 2.0, 25.0, 3.0, 0.1, 11.0, 10.5]), 10.0, 2, 6)
    assert pg["above"].tolist() == [2, 5, 6] and pg["rows"].tolist() == [0, 1, 4]
    assert pg["comp"].tolist() == [True, True, True, False, False, False] and pg["weight"].tolist() == [50.0, 60.0, 90.0]
    # 0-1 above: image 1 stays joined through 1-2; the bound itself (10.0) is not above
    pg = positioning_graph(vg, use, np.array([10.1, 10.0, 0.5, 3.0, 0.1, 4.0, 1.0]), 10.0, 0, 6)
    assert pg["above"].tolist() == [0] and pg["rows"].tolist() == [1, 2, 3, 4, 5, 6] and pg["comp"].tolist() == [True] * 5 + [False]
    # every pair of the root above: the root is alone
    pg = positioning_graph(vg, use, np.array([20.0, 1.0, 1.0, 1.0, 20.0, 1.0, 1.0]), 10.0, 0, 6)
    assert pg["comp"].tolist() == [True] + [False] * 5 and pg["rows"].tolist() == [] and pg["weight"].tolist() == []
