"""Global mapping on the GPU: pxr_rotation_averaging and pxr_global_positioning (csrc/pxr_global.hip) against the numpy references of
tests/global_mapping_cases.py -- same comparisons and bounds as the lane test: integers and statuses equal, floating outputs within
global_mapping_cases.bound() --, two runs bit for bit, the classes of PXR_EINVAL, and GlobalMapper end to end.

Bounds of the end-to-end tests (the rule tests/test_mapping_gpu.py applies to the incremental mapper): the mean reprojection error
may exceed the known-pose pipeline's (ground-truth poses, TrackTriangulator, geometric bundle adjustment) by 5 %, and after a
similarity alignment the rotation and centre errors may be twice that pipeline's own."""
import ctypes as C

import numpy as np
import pytest

import global_mapping_cases as gc
import mapping_cases as mc

pytestmark = pytest.mark.gpu
_CACHE = {}


# ---- the two entry points on device copies ----------------------------------------------------------------------------------------
def _check(rc, name):
    from pixsfm_amd._lib import check
    check(rc, name)


def run_rotavg(ctx, n_images, pair_image, pair_qvec, pair_weight, **options):
    from pixsfm_amd.engine import rotavg_options
    pim = np.ascontiguousarray(pair_image, np.int32).reshape(-1, 2)
    d = [ctx.to_device(pim, np.int32), ctx.to_device(pair_qvec, np.float64), ctx.to_device(pair_weight, np.float64)]
    out = dict(qvec=ctx.to_device(np.full((n_images, 4), -9.0)), pair_angle=ctx.to_device(np.full(len(pim), -9.0)))
    opts = rotavg_options(**options)
    root, iterations = C.c_int32(-9), C.c_int32(-9)
    rc = ctx.lib.pxr_rotation_averaging(ctx.handle, n_images, len(pim), d[0].ptr, d[1].ptr, d[2].ptr, C.byref(opts), out["qvec"].ptr,
                                        C.byref(root), C.byref(iterations), out["pair_angle"].ptr)
    res = {k: v.download() for k, v in out.items()}
    res.update(root=root.value, iterations=iterations.value)
    try:
        _check(rc, "pxr_rotation_averaging")
    except Exception as err:
        err.outputs = res
        raise
    return res


def run_positioning(ctx, scene, qvec, pair_image, pair_dir, pair_weight, root, **options):
    from pixsfm_amd import _lib
    from pixsfm_amd.engine import _padded_cam_params, globalpos_options
    pim = np.ascontiguousarray(pair_image, np.int32).reshape(-1, 2)
    n_cam = len(scene["cam_model"])
    d = dict(off=ctx.to_device(scene["track_offsets"], np.int64), img=ctx.to_device(scene["obs_image"], np.int32),
             xy=ctx.to_device(scene["obs_xy"], np.float64), icam=ctx.to_device(scene["image_camera"], np.int32),
             q=ctx.to_device(qvec, np.float64), model=ctx.to_device(scene["cam_model"], np.int32),
             params=ctx.to_device(_padded_cam_params(scene["cam_params"], n_cam), np.float64), pim=ctx.to_device(pim, np.int32),
             pd=ctx.to_device(pair_dir, np.float64), pw=ctx.to_device(pair_weight, np.float64))
    T, N, n = len(scene["track_offsets"]) - 1, len(scene["obs_image"]), len(scene["image_camera"])
    view = _lib.TriView(T, d["off"].ptr, N, d["img"].ptr, d["xy"].ptr, n, d["icam"].ptr, d["q"].ptr, None, n_cam, d["model"].ptr, d["params"].ptr)
    out = dict(centre=ctx.to_device(np.full((n, 3), -9.0)), xyz=ctx.to_device(np.full((T, 3), -9.0)),
               track_status=ctx.to_device(np.full(T, -9, np.int32)), obs_weight=ctx.to_device(np.full(N, -9.0)),
               pair_weight=ctx.to_device(np.full(len(pim), -9.0)))
    opts = globalpos_options(**options)
    status, rounds = C.c_int32(-9), C.c_int32(-9)
    rc = ctx.lib.pxr_global_positioning(ctx.handle, C.byref(view), len(pim), d["pim"].ptr, d["pd"].ptr, d["pw"].ptr, int(root), C.byref(opts),
                                        out["centre"].ptr, out["xyz"].ptr, out["track_status"].ptr, out["obs_weight"].ptr,
                                        out["pair_weight"].ptr, C.byref(status), C.byref(rounds))
    res = {k: v.download() for k, v in out.items()}
    res.update(status=status.value, rounds=rounds.value)
    try:
        _check(rc, "pxr_global_positioning")
    except Exception as err:
        err.outputs = res
        raise
    return res


def _solved(name, n_images=None):
    return gc.solved(name, n_images)


@pytest.mark.parametrize("case", [("boundary", n) for n in gc.LAPLACIAN_SIZES] + [("ring40", None)])
def test_rotation_averaging_matches_the_reference(ctx, case):
    scene, ref, _, _ = _solved(*case)
    got = run_rotavg(ctx, len(scene["image_camera"]), scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    gc.within_bounds(gc.compare_rotavg(got, ref))


@pytest.mark.parametrize("case", [("boundary", n) for n in gc.POSITIONING_SIZES] + [("ring40", None)])
def test_positioning_matches_the_reference(ctx, case):
    scene, ra, b, ref = _solved(*case)
    got = run_positioning(ctx, scene, ra["qvec"], scene["pair_image"], b, scene["pair_weight"], ra["root"])
    gc.within_bounds(gc.compare_positioning(got, ref))


def test_two_runs_give_identical_bits_in_every_output(ctx):
    scene, ra, b, _ = _solved("ring40")
    runs = [(run_rotavg(ctx, 40, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"]),
             run_positioning(ctx, scene, ra["qvec"], scene["pair_image"], b, scene["pair_weight"], ra["root"])) for _ in range(2)]
    for a, c in zip(runs[0], runs[1]):
        for k in a:
            assert np.array_equal(a[k], c[k], equal_nan=True), k


def test_timed_twins_and_engine_wrappers(ctx):
    """The engine classes give the results of the plain calls, and their timed twins one time per stage."""
    from pixsfm_amd.engine import GlobalPositioningProblem, RotationAveragingProblem
    scene, ra, b, ref = _solved("boundary", 23)
    prob = RotationAveragingProblem(ctx, 23, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    d_q, root, iterations, d_angle = prob.solve(timed=True)
    assert root == ra["root"] and iterations == ra["iterations"] and set(prob.kernel_ms) == {"residuals", "assembly", "solve"}
    assert np.abs(d_q.download() - ra["qvec"]).max() <= gc.bound("qvec")
    gp = GlobalPositioningProblem(ctx, dict(scene, qvec=ra["qvec"]), scene["pair_image"], b, scene["pair_weight"], ra["root"])
    out = gp.solve(timed=True)
    print("kernel ms:", prob.kernel_ms, gp.kernel_ms)
    assert out["status"] == 0 and out["rounds"] == 8 and set(gp.kernel_ms) == {"tracks", "contraction", "gauge_pack", "cholesky", "update"}
    assert np.abs(out["centre"].download() - ref["centre"]).max() <= gc.bound("centre")
    assert np.array_equal(out["track_status"].download(), ref["track_status"])


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(ctx):
    from pixsfm_amd._lib import PixsfmHipError
    scene, ra, b, _ = _solved("boundary", 22)
    n = len(scene["image_camera"])
    for name, key, bad, word in gc.bad_rotation_inputs(scene):
        a = dict(pair_image=scene["pair_image"], pair_qvec=scene["pair_qvec"], pair_weight=scene["pair_weight"])
        a[key] = bad
        if key == "pair_image" and len(bad) != len(scene["pair_image"]):
            a["pair_qvec"], a["pair_weight"] = scene["pair_qvec"][:len(bad)], scene["pair_weight"][:len(bad)]
        with pytest.raises(PixsfmHipError, match=word) as e:
            run_rotavg(ctx, n, a["pair_image"], a["pair_qvec"], a["pair_weight"])
        assert e.value.code == -1 and gc.untouched(e.value.outputs), name                       # PXR_EINVAL
    for name, key, bad, word in gc.bad_positioning_inputs(scene, b):
        sc, a = dict(scene), dict(pair_image=scene["pair_image"], pair_dir=b, pair_weight=scene["pair_weight"], root=ra["root"])
        if key in a:
            a[key] = bad
        else:
            sc[key] = bad
        with pytest.raises(PixsfmHipError, match=word) as e:
            run_positioning(ctx, sc, ra["qvec"], a["pair_image"], a["pair_dir"], a["pair_weight"], a["root"])
        assert e.value.code == -1 and gc.untouched(e.value.outputs), name
    # one image beyond the dense solves: 1002 images for either entry point
    with pytest.raises(PixsfmHipError, match="PXR_MAX_IMAGES_DIRECT") as e:
        run_rotavg(ctx, 1002, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    assert e.value.code == -1 and gc.untouched(e.value.outputs)
    big = dict(scene, image_camera=np.zeros(1002, np.int32))
    with pytest.raises(PixsfmHipError, match="PXR_MAX_IMAGES_DIRECT") as e:
        run_positioning(ctx, big, np.tile([1.0, 0.0, 0.0, 0.0], (1002, 1)), scene["pair_image"], b, scene["pair_weight"], ra["root"])
    assert e.value.code == -1 and gc.untouched(e.value.outputs)
    # and 1001 images pass the size check: they are refused for what is checked after it
    with pytest.raises(PixsfmHipError, match="not connected") as e:
        run_rotavg(ctx, 1001, scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    assert e.value.code == -1 and gc.untouched(e.value.outputs)


# ---- GlobalMapper ------------------------------------------------------------------------------------------------------------------
def _inputs(kind):
    """(scene, pairs, matches, graph, labels) of scene A, a trap of tests/mapping_cases.py, or the low-parallax ring."""
    if ("in", kind) not in _CACHE:
        scene = dict(A=lambda: mc.ring_scene(seed=0), split=lambda: mc.ring_scene(n_images_second=4, unmatched=1, seed=0),
                     wrong=lambda: mc.ring_scene(wrong_share=0.1, seed=mc.WRONG_SEED), low=lambda: gc.low_parallax_ring()[0])[kind]()
        pairs, matches = mc.matches_from_labels(scene)
        graph, labels = mc.graph_and_labels(scene, pairs, matches)
        _CACHE["in", kind] = (scene, pairs, matches, graph, labels)
    return _CACHE["in", kind]


def _geometries(ctx, kind):
    if ("geom", kind) not in _CACHE:
        from pixsfm_amd.api import TwoViewVerifier
        scene, pairs, matches, _, _ = _inputs(kind)
        _CACHE["geom", kind] = TwoViewVerifier.create({}, ctx=ctx).verify_pairs(scene["keypoints"], scene["cameras"], pairs, matches)[2]
    return _CACHE["geom", kind]


def _map(ctx, kind, geometries=None, conf=None):
    from pixsfm_amd.api import GlobalMapper
    scene, pairs, _, graph, labels = _inputs(kind)
    return GlobalMapper.create(conf, ctx=ctx).reconstruct(scene["cameras"], scene["keypoints"], graph, pairs,
                                                        _geometries(ctx, kind) if geometries is None else geometries, track_labels=labels)


def _known_pose_figures(ctx, kind, gauge_names):
    """(mean reprojection error, max rotation error, max centre error) of the known-pose pipeline with the mapper's gauge."""
    if ("ref", kind) not in _CACHE:
        from pixsfm_amd.api import BundleAdjustmentSetup, GeometricBundleOptimizer, TrackTriangulator
        from pixsfm_amd.api.mapping import gauge_component
        from pixsfm_amd.api.reconstruction import Image, Reconstruction
        from pixsfm_amd.api.triangulation import mean_reprojection_error
        scene, _, _, graph, labels = _inputs(kind)
        rec, ids = Reconstruction(), {}
        rec.add_camera(scene["camera"])
        for k, nm in enumerate(scene["names"]):
            ids[nm] = k + 1
            rec.add_image(Image(k + 1, nm, 1, *scene["poses"][nm]))
        model, _ = TrackTriangulator.create({}, ctx=ctx).triangulate(rec, scene["keypoints"], graph, track_labels=labels)
        setup = BundleAdjustmentSetup()
        setup.add_images(model.reg_image_ids())
        setup.set_constant_pose(ids[gauge_names[0]])
        setup.set_constant_tvec(ids[gauge_names[1]], [gauge_component(model.images[ids[gauge_names[1]]].tvec)])
        setup.set_constant_camera(1)
        GeometricBundleOptimizer({'loss': {'name': 'trivial', 'params': []}, 'solver': {'max_num_iterations': 50}, 'print_summary': False},
                                 setup, ctx=ctx).run(model)
        _CACHE["ref", kind] = (mean_reprojection_error(ctx, model),) + mc.pose_errors(model, scene["poses"])
    return _CACHE["ref", kind]


def _within_the_pose_error_rule(ctx, kind, rec, summary):
    from pixsfm_amd.api.triangulation import mean_reprojection_error
    scene = _inputs(kind)[0]
    e_ref, rot_ref, cen_ref = _known_pose_figures(ctx, kind, (summary["root"], summary["gauge_image"]))
    e_map, (rot_map, cen_map) = mean_reprojection_error(ctx, rec), mc.pose_errors(rec, scene["poses"])
    print("global mapper: %d images, %d points, mean reprojection error %.6f px, max rotation error %.6f deg, max centre error %.6f"
          % (len(rec.images), len(rec.points3D), e_map, rot_map, cen_map))
    print("known-pose pipeline: mean reprojection error %.6f px, max rotation error %.6f deg, max centre error %.6f" % (e_ref, rot_ref, cen_ref))
    print({k: summary[k] for k in ("rotation_iterations", "residual_histogram", "positioning_rounds", "zero_weight_observations",
                                   "zero_weight_pairs", "kernel_ms")})
    assert e_map <= 1.05 * e_ref
    assert rot_map <= 2.0 * rot_ref and cen_map <= 2.0 * cen_ref


def test_scene_a_registers_all_images(ctx):
    rec, summary = _map(ctx, "A")
    assert summary["status"] == "ok" and summary["num_reg_images"] == 10 and summary["unregistered"] == []
    assert len(rec.images) == 10 and len(rec.points3D) > 250
    _within_the_pose_error_rule(ctx, "A", rec, summary)


def test_rotation_averaging_of_the_api_on_scene_a(ctx):
    """api.rotation_averaging(names, pairs, geometries): the rotations GlobalMapper averages, by name, against ground truth in the
    root's frame -- within 1 degree, the condition the reference is held to on far worse pairs --, the root GlobalMapper reports,
    and one residual per pair used: the pairs with a geometry, all of them far below max_rotation_residual.  Two images without
    pairs are not in the result."""
    from pixsfm_amd.api import rotation_averaging
    from pixsfm_amd.synthetic import qvec_to_rotmat
    scene, pairs, _, _, _ = _inputs("A")
    geoms = _geometries(ctx, "A")
    names = ["nobody0.jpg"] + scene["names"] + ["nobody1.jpg"]                       # the component must be re-indexed
    qvec, root, residual = rotation_averaging(names, pairs, geoms, ctx=ctx)
    _, summary = _map(ctx, "A")
    assert root == summary["root"] and sorted(qvec) == sorted(scene["names"])
    assert sorted(residual) == sorted(tuple(p) for p, g in zip(pairs, geoms) if g.get("success"))
    assert max(residual.values()) < 2.0 and np.allclose(qvec[root], [1.0, 0.0, 0.0, 0.0])
    R_root = qvec_to_rotmat(scene["poses"][root][0])
    worst = 0.0
    for nm in scene["names"]:
        dR = qvec_to_rotmat(qvec[nm]) @ (qvec_to_rotmat(scene["poses"][nm][0]) @ R_root.T).T
        worst = max(worst, np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
    print("root %s, %d pairs, largest residual %.3f deg, max rotation error %.3f deg" % (root, len(residual), max(residual.values()), worst))
    assert worst <= 1.0
    with pytest.raises(ValueError):
        rotation_averaging(names, pairs, geoms, conf={'no_such_key': 1}, ctx=ctx)


def test_low_parallax_ring_defeats_the_incremental_mapper_and_not_the_global_one(ctx):
    """The test that cannot pass without the feature: on the smallest ring on which no pair passes the initial-pair criteria the
    incremental mapper ends in no_initial_pair; the global mapper registers every image within the pose-error rule."""
    from pixsfm_amd.api import IncrementalMapper
    scene, pairs, _, graph, labels = _inputs("low")
    assert gc.initial_pair_candidates(scene) == []
    _, inc = IncrementalMapper.create(None, ctx=ctx).reconstruct(scene["cameras"], scene["keypoints"], graph, pairs, _geometries(ctx, "low"),
                                                                track_labels=labels)
    assert inc["status"] == "no_initial_pair" and inc["num_reg_images"] == 0
    rec, summary = _map(ctx, "low")
    assert summary["status"] == "ok" and summary["unregistered"] == [] and len(rec.images) == len(scene["names"])
    _within_the_pose_error_rule(ctx, "low", rec, summary)


def test_unmatched_image_and_second_component_stay_unregistered(ctx):
    scene = _inputs("split")[0]
    rec, summary = _map(ctx, "split")
    assert summary["status"] == "ok" and summary["unregistered"] == scene["names"][10:]
    assert sorted(im.name for im in rec.images.values()) == scene["names"][:10]


def test_members_of_wrong_tracks_do_not_survive(ctx):
    scene = _inputs("wrong")[0]
    rec, summary = _map(ctx, "wrong")
    assert summary["num_reg_images"] == 10 and summary["unregistered"] == []
    by_name = {im.name: im for im in rec.images.values()}
    n_wrong = 0
    for nm in scene["names"]:
        for f in np.flatnonzero(scene["wrong"][nm]):
            n_wrong += 1
            assert by_name[nm].points2D[f].point3D_id == -1, (nm, f)
    print("%d members of wrong tracks, none in a final track; %d points" % (n_wrong, len(rec.points3D)))


def test_random_geometries_are_reported_and_change_nothing(ctx):
    """A tenth of the verified geometries replaced by random poses: every one of them ends above max_rotation_residual, and the
    model stays within the pose-error rule."""
    scene, pairs, _, _, _ = _inputs("A")
    rng = np.random.default_rng(4)
    geoms = [dict(g) for g in _geometries(ctx, "A")]
    good = [p for p, g in enumerate(geoms) if g.get("success")]
    bad = [good[k] for k in rng.permutation(len(good))[:max(len(good) // 10, 1)]]
    for p in bad:
        q, t = rng.normal(size=4), rng.normal(size=3)
        geoms[p].update(qvec=q / np.linalg.norm(q), tvec=t / np.linalg.norm(t))
    rec, summary = _map(ctx, "A", geometries=geoms)
    assert set(summary["pairs_above_max_residual"]) == {tuple(pairs[p]) for p in bad}
    assert summary["num_reg_images"] == 10
    _within_the_pose_error_rule(ctx, "A", rec, summary)


def test_panoramic_pair_gives_a_rotation_and_no_baseline(ctx):
    scene, pairs, _, _, _ = _inputs("A")
    geoms = [dict(g, config="CALIBRATED") if g.get("success") else dict(g) for g in _geometries(ctx, "A")]
    p = [k for k, g in enumerate(geoms) if g.get("success")][3]
    geoms[p]["config"] = "PANORAMIC"
    rec, summary = _map(ctx, "A", geometries=geoms)
    assert summary["panoramic_pairs"] == [tuple(pairs[p])] and tuple(pairs[p]) not in summary["pairs_above_max_residual"]
    weights = summary["positioning_pairs"]
    assert weights[tuple(pairs[p])] == 0.0 and sum(w > 0.0 for w in weights.values()) >= len(weights) - 3
    assert summary["num_reg_images"] == 10
