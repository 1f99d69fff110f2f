"""SiftExtractor end to end on the GPU: two rendered views of a golden tile with known cameras -> extract_images ->
DescriptorMatcher("NN-ratio"), against the numpy reference of tests/sift_cases.py run on the same views and matched by numpy
brute force with the same ratio; then max_num_features, device arrays into features_from_image_list(device=True) and one
keypoint adjustment, the coordinate convention, and the configuration errors."""
import numpy as np
import pytest

import real_scene as rs
import sift_cases as sc

pytestmark = pytest.mark.gpu

CONF = dict(first_octave=0)            # the views are 320 x 320; one octave less keeps the float64 reference at about a second per view
RATIO = 0.8                            # "NN-ratio"


@pytest.fixture(scope="module")
def ctx():
    from pixsfm_amd.engine import Context
    return Context(0)


@pytest.fixture(scope="module")
def views(tmp_path_factory):
    """Two grey views written as PNGs (mode L, so the file's pixels are the detector's input), their cameras."""
    from PIL import Image
    Rs, ts = rs.cameras(2, 3)
    tile = rs.load_tile(0)
    d = tmp_path_factory.mktemp("sift_views")
    names, greys = [], []
    for v in range(2):
        g = np.round(rs.render_view(tile, Rs[v], ts[v]).mean(0)).astype(np.uint8)
        names.append("view%d.png" % v)
        Image.fromarray(g).save(str(d / names[-1]))
        greys.append(g)
    return str(d), names, greys, Rs, ts


def plane_map(kp, Ra, ta, Rb, tb):
    """COLMAP pixels of view a -> the plane z = 0 -> COLMAP pixels of view b."""
    d = np.stack([(kp[:, 0] - rs.VIEW / 2) / rs.FOCAL, (kp[:, 1] - rs.VIEW / 2) / rs.FOCAL, np.ones(len(kp))], -1) @ Ra
    c = -Ra.T @ ta
    X = c + (-c[2] / d[:, 2])[:, None] * d
    p = X @ Rb.T + tb
    return np.stack([rs.FOCAL * p[:, 0] / p[:, 2] + rs.VIEW / 2, rs.FOCAL * p[:, 1] / p[:, 2] + rs.VIEW / 2], -1)


def brute_force_ratio(A, B, ratio):
    """Mutual nearest neighbours with Lowe's ratio on distances, in float64: (M, 2) indices."""
    sim = A @ B.T

    def one_way(s):
        best = s.argmax(1)
        s1 = s[np.arange(len(s)), best]
        s2 = np.where(np.arange(s.shape[1])[None, :] == best[:, None], -np.inf, s).max(1)
        ok = 2.0 * (1.0 - s1) <= ratio * ratio * 2.0 * (1.0 - s2)
        return np.where(ok, best, -1)
    m0, m1 = one_way(sim), one_way(sim.T)
    idx = np.nonzero(m0 >= 0)[0]
    idx = idx[m1[m0[idx]] == idx]
    return np.stack([idx, m0[idx]], -1)


def correct(matches, kp_a, kp_b, cams):
    Rs, ts = cams
    if len(matches) == 0:
        return 0
    err = np.linalg.norm(plane_map(kp_a[matches[:, 0]], Rs[0], ts[0], Rs[1], ts[1]) - kp_b[matches[:, 1]], axis=1)
    return int((err <= 3.0).sum())


@pytest.fixture(scope="module")
def extracted(ctx, views):
    from pixsfm_amd.api import SiftExtractor
    d, names, _, _, _ = views
    return SiftExtractor.create(CONF, ctx=ctx).extract_images(d, names)


def test_matches_of_two_views_against_the_reference(ctx, views, extracted):
    """A match is correct if it lies within 3 px of the plane-induced mapping.  The bar is the reference's own figure: the GPU path
    must reach 0.9 x its number of correct matches (the two differ only by the margin cases, <= 5 % per image, hence 10 % per
    pair) and a precision no more than 0.02 below the reference's."""
    from pixsfm_amd.api import DescriptorMatcher
    d, names, greys, Rs, ts = views
    keypoints, descriptors = extracted
    matches, _ = DescriptorMatcher.create("NN-ratio", ctx=ctx).match_pairs(descriptors, [(names[0], names[1])])
    m = matches[0].astype(np.int64)
    got = correct(m, keypoints[names[0]], keypoints[names[1]], (Rs, ts))
    ref = [sc.extract(g, **CONF)[0] for g in greys]
    kp_ref = [f["keypoints"][:, :2] + 0.5 for f in ref]
    m_ref = brute_force_ratio(ref[0]["descriptors"], ref[1]["descriptors"], RATIO)
    want = correct(m_ref, kp_ref[0], kp_ref[1], (Rs, ts))
    print("features %d / %d (reference %d / %d), matches %d (reference %d), correct %d (reference %d)"
          % (len(keypoints[names[0]]), len(keypoints[names[1]]), len(kp_ref[0]), len(kp_ref[1]), len(m), len(m_ref), got, want))
    assert want >= 30
    assert got >= 0.9 * want
    assert got / max(len(m), 1) >= want / max(len(m_ref), 1) - 0.02


def test_coordinate_convention_and_outputs(ctx, views, extracted):
    """The Python layer returns COLMAP coordinates (the C-ABI's pixel indices + 0.5), float32 unit descriptors, one row each."""
    from pixsfm_amd.api import SiftExtractor
    from pixsfm_amd.engine import SiftPyramid
    d, names, greys, _, _ = views
    keypoints, descriptors = extracted
    r = SiftExtractor.create(CONF, ctx=ctx).extract(greys[0])
    assert np.array_equal(r["keypoints"], keypoints[names[0]]) and np.array_equal(r["descriptors"], descriptors[names[0]])
    n = len(r["keypoints"])
    assert r["keypoints"].shape == (n, 2) and r["scales"].shape == (n,) and r["orientations"].shape == (n,) and r["scores"].shape == (n,)
    assert r["descriptors"].shape == (n, 128) and r["descriptors"].dtype == np.float32
    assert np.abs(np.linalg.norm(r["descriptors"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    pyr = SiftPyramid(ctx, greys[0], **CONF)
    kp = pyr.detect()[0].download()
    assert np.array_equal(r["keypoints"], kp[:, :2] + 0.5) and np.array_equal(r["scales"], kp[:, 2]) and np.array_equal(r["orientations"], kp[:, 3])
    # describe() of the returned keypoints gives the same descriptors back
    desc, valid = SiftExtractor.create(CONF, ctx=ctx).describe(greys[0], r["keypoints"], r["scales"], r["orientations"])
    assert valid.all() and np.abs(desc - r["descriptors"]).max() <= 1e-6        # ((x + 0.5) - 0.5 may differ from x in the last bit)


def test_max_num_features_keeps_the_largest_scales(ctx, views, extracted):
    from pixsfm_amd.api import SiftExtractor
    _, names, greys, _, _ = views
    full = SiftExtractor.create(CONF, ctx=ctx).extract(greys[0])
    n = len(full["scales"])
    few = SiftExtractor.create(dict(CONF, max_num_features=n // 3), ctx=ctx).extract(greys[0])
    keep = np.sort(np.argsort(-full["scales"], kind="stable")[:n // 3])
    assert len(few["scales"]) == n // 3
    for k in ("keypoints", "scales", "orientations", "scores", "descriptors"):
        assert np.array_equal(few[k], full[k][keep]), k
    same = SiftExtractor.create(dict(CONF, max_num_features=n + 5), ctx=ctx).extract(greys[0])
    assert np.array_equal(same["descriptors"], full["descriptors"])


def test_device_arrays_into_the_extractor_and_one_keypoint_adjustment(ctx, views):
    """device=True returns device arrays; they go into features_from_image_list(device=True) and the matcher as they are, and a
    keypoint adjustment over the matched keypoints runs."""
    from pixsfm_amd.api import DescriptorMatcher, FeatureExtractor, SiftExtractor, features_from_image_list
    from pixsfm_amd.engine import DeviceArray, interp_cfg, lm_options, make_loss
    from pixsfm_amd.ka_engine import KAProblem
    d, names, greys, _, _ = views
    keypoints, descriptors = SiftExtractor.create(dict(CONF, device=True, max_num_features=300), ctx=ctx).extract_images(d, names)
    assert all(isinstance(v, DeviceArray) for v in list(keypoints.values()) + list(descriptors.values()))
    matches, _ = DescriptorMatcher.create("NN-ratio", ctx=ctx).match_pairs(descriptors, [(names[0], names[1])])
    m = matches[0].astype(np.int64)
    assert len(m) >= 20
    ex = FeatureExtractor({"model": {"name": "dsift"}, "max_edge": 2000}, ctx=ctx)
    fm = features_from_image_list(ex, d, names, keypoints=keypoints, device=True)
    arena = fm.fset(0).arena
    n0 = keypoints[names[0]].shape[0]
    assert arena.n == n0 + keypoints[names[1]].shape[0]
    kp = np.concatenate([np.asarray(keypoints[names[0]])[m[:, 0]], np.asarray(keypoints[names[1]])[m[:, 1]]])
    k = len(m)
    prob = dict(kp=kp.copy(), node_patch=np.concatenate([m[:, 0], n0 + m[:, 1]]).astype(np.int64),
                node_const=np.concatenate([np.ones(k), np.zeros(k)]).astype(np.uint8),
                node_problem=np.concatenate([np.arange(k) // 25, np.arange(k) // 25]).astype(np.int32),
                edge_src=np.arange(k, dtype=np.int64), edge_dst=np.arange(k, 2 * k, dtype=np.int64), edge_w=np.ones(k))
    ka = KAProblem(ctx, arena, prob)
    total, _ = ka.solve(interp_cfg(), make_loss("cauchy", [0.25]), bound=4.0, options=lm_options(parameter_tolerance=1e-5), per_problem=True)
    moved = ka.keypoints()
    assert total["final_cost"] <= total["initial_cost"] and np.isfinite(moved).all()
    assert np.array_equal(moved[:k], kp[:k]) and np.abs(moved - kp).max() <= 4.0 + 1e-9


def test_configuration_errors(ctx):
    from pixsfm_amd.api import SiftExtractor
    from pixsfm_amd.engine import sift_options
    with pytest.raises(ValueError, match="unknown configuration key"):
        SiftExtractor.create({"octaves": 3}, ctx=ctx)
    with pytest.raises(ValueError, match="normalization"):
        SiftExtractor.create({"normalization": "L1"}, ctx=ctx)
    with pytest.raises(ValueError, match="max_num_features"):
        SiftExtractor.create({"max_num_features": -1}, ctx=ctx)
    with pytest.raises(ValueError, match="unknown SIFT option"):
        sift_options(octaves=3)
    with pytest.raises(ValueError, match="image must be"):
        SiftExtractor.create(ctx=ctx).extract(np.zeros((4, 5, 2), np.uint8))
    from pixsfm_amd._lib import PixsfmHipError
    with pytest.raises(PixsfmHipError, match="octave_resolution"):
        SiftExtractor.create({"octave_resolution": 7}, ctx=ctx).extract(np.zeros((40, 50), np.uint8))
