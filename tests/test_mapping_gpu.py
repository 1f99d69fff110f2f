"""Incremental mapping on the GPU: pxr_mapper_visibility (csrc/pxr_mapper.hip) bit for bit against the numpy reference of
tests/mapping_cases.py, its hand-over to pxr_absolute_pose, and IncrementalMapper end to end against the known-pose pipeline
(TrackTriangulator with ground-truth poses + geometric bundle adjustment with the same gauge) on ring scenes.

Bounds of the end-to-end tests (set by the issue that introduced the mapper): the mapper's mean reprojection error may exceed
the known-pose pipeline's by 5 % -- both minimise one cost over the same observations up to their inlier sets, so more is a
wrong minimum; after similarity alignment its rotation and centre errors may be twice the known-pose pipeline's own, whose
poses drift with the same keypoint noise."""
import numpy as np
import pytest

import mapping_cases as mc

pytestmark = pytest.mark.gpu

OUTPUTS = ("n_visible", "score", "corr_offsets", "corr_obs", "corr_xy", "corr_xyz")
_CACHE = {}


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _scene_on_device(ctx):
    from pixsfm_amd.engine import MapperScene
    scene, xyz, status, mask, planned = mc.boundary_batch()
    return MapperScene(ctx, scene), ctx.to_device(xyz, np.float64), ctx.to_device(status, np.int32)


@pytest.mark.parametrize("levels", [1, 6])
def test_visibility_matches_the_reference_bit_for_bit(ctx, levels):
    scene, xyz, status, mask, planned = mc.boundary_batch()
    ref = mc.visibility_reference(scene, xyz, status, mask, levels)
    assert ref["n_visible"].tolist() == planned.tolist()
    s, d_xyz, d_status = _scene_on_device(ctx)
    got = s.visibility(d_xyz, d_status, mask, levels, timed=(levels == 6))
    assert got["n_corr"] == ref["n_corr"]
    for k in OUTPUTS:
        a = got[k].download()
        assert np.array_equal(a if k in OUTPUTS[:3] else a[:ref["n_corr"]], ref[k]), k
    if levels == 6:
        print("kernel ms:", s.kernel_ms)
        assert set(s.kernel_ms) == {"check", "count", "scan", "write"}


@pytest.mark.parametrize("n_images", [255, 256, 257, 600])
def test_offsets_over_many_images_match_the_reference(ctx, n_images):
    """More images than the boundary batch's 11: the prefix sum of the visible counts (k_exclusive_scan<256> of csrc/pxr_scan.h) at
    one image to a thread less one, exactly, a second image on the first threads, and three to a thread."""
    from pixsfm_amd.engine import MapperScene
    scene, xyz, status, mask = mc.many_images_batch(n_images)
    ref = mc.visibility_reference(scene, xyz, status, mask, 3)
    got = MapperScene(ctx, scene).visibility(ctx.to_device(xyz, np.float64), ctx.to_device(status, np.int32), mask, 3)
    assert got["n_corr"] == ref["n_corr"] > n_images
    for k in OUTPUTS:
        a = got[k].download()
        assert np.array_equal(a if k in OUTPUTS[:3] else a[:ref["n_corr"]], ref[k]), k


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(ctx):
    from pixsfm_amd._lib import PixsfmHipError
    scene, xyz, status, mask, _ = mc.boundary_batch()
    s, d_xyz, d_status = _scene_on_device(ctx)
    n_images, n_obs = s.n_images, s.n_obs
    fill = dict(n_visible=np.full(n_images, -9, np.int32), score=np.full(n_images, -9, np.int64),
                corr_offsets=np.full(n_images + 1, -9, np.int64), corr_obs=np.full(n_obs, -9, np.int64),
                corr_xy=np.full((n_obs, 2), -9.0), corr_xyz=np.full((n_obs, 3), -9.0))
    out = {k: ctx.to_device(v) for k, v in fill.items()}
    host = dict(track_offsets=s.track_offsets, obs_image=s.obs_image, obs_track=s.obs_track, image_obs_offsets=s.image_obs_offsets,
                image_obs=s.image_obs, image_camera=s.image_camera, cam_size=s.cam_size)
    for name, key, bad, word in mc.bad_inputs(scene):
        s.d[key].upload(bad)
        with pytest.raises(PixsfmHipError, match=word) as e:
            s.visibility(d_xyz, d_status, mask, 6, out=out)
        assert e.value.code == -1, name                                     # PXR_EINVAL
        s.d[key].upload(host[key])
    for levels in (0, 7):
        with pytest.raises(PixsfmHipError, match="pyramid_levels") as e:
            s.visibility(d_xyz, d_status, mask, levels, out=out)
        assert e.value.code == -1
    for k, v in fill.items():
        assert np.array_equal(out[k].download(), v), k
    ref = mc.visibility_reference(scene, xyz, status, mask, 6)             # and the scene still works once every array is back
    assert np.array_equal(s.visibility(d_xyz, d_status, mask, 6, out=out)["score"].download(), ref["score"])


# ---- scenes, the mapper and the known-pose pipeline -------------------------------------------------------------------------------
def _inputs(kind):
    """(scene, pairs, graph, labels) of a trap or of scene A; geometries are added by _geometries (they need the GPU)."""
    if ("in", kind) not in _CACHE:
        scene = dict(A=lambda: mc.ring_scene(seed=0), split=lambda: mc.ring_scene(n_images_second=4, unmatched=1, seed=0),
                     cocentred=lambda: mc.ring_scene(cocentred=True, seed=0), wrong=lambda: mc.ring_scene(wrong_share=0.1, seed=mc.WRONG_SEED))[kind]()
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


def _map(ctx, kind, conf=None, fresh=False):
    key = ("map", kind, repr(conf))
    if fresh or key not in _CACHE:
        from pixsfm_amd.api import IncrementalMapper
        scene, pairs, _, graph, labels = _inputs(kind)
        out = IncrementalMapper.create(conf, ctx=ctx).reconstruct(scene["cameras"], scene["keypoints"], graph, pairs,
                                                                 _geometries(ctx, kind), track_labels=labels)
        if fresh:
            return out
        _CACHE[key] = out
    return _CACHE[key]


def _known_pose_pipeline(ctx, kind, init_names, refine=True):
    """The same keypoints and tracks with ground-truth poses: TrackTriangulator, then (refine) geometric bundle adjustment with
    the mapper's gauge.  Returns (Reconstruction, triangulation summary)."""
    from pixsfm_amd.api import BundleAdjustmentSetup, GeometricBundleOptimizer, TrackTriangulator
    from pixsfm_amd.api.mapping import gauge_component
    from pixsfm_amd.api.reconstruction import Image, Reconstruction
    scene, _, _, graph, labels = _inputs(kind)
    rec = Reconstruction()
    rec.add_camera(scene["camera"])
    ids = {}
    for k, nm in enumerate(scene["names"]):
        ids[nm] = k + 1
        rec.add_image(Image(k + 1, nm, 1, *scene["poses"][nm]))
    model, summary = TrackTriangulator.create({}, ctx=ctx).triangulate(rec, scene["keypoints"], graph, track_labels=labels)
    if refine:
        setup = BundleAdjustmentSetup()
        setup.add_images(model.reg_image_ids())
        setup.set_constant_pose(ids[init_names[0]])
        setup.set_constant_tvec(ids[init_names[1]], [gauge_component(model.images[ids[init_names[1]]].tvec)])
        setup.set_constant_camera(1)
        options = {'loss': {'name': 'trivial', 'params': []}, 'solver': {'max_num_iterations': 50}, 'print_summary': False}
        GeometricBundleOptimizer(options, setup, ctx=ctx).run(model)
    return model, summary


def _check_against_known_poses(ctx, kind, rec, summary):
    from pixsfm_amd.api.triangulation import mean_reprojection_error
    scene = _inputs(kind)[0]
    if ("ref", kind) not in _CACHE:
        ref, _ = _known_pose_pipeline(ctx, kind, summary["initial_pair"])
        _CACHE["ref", kind] = (mean_reprojection_error(ctx, ref),) + mc.pose_errors(ref, scene["poses"]) + (len(ref.points3D),)
    e_ref, rot_ref, cen_ref, n_ref = _CACHE["ref", kind]
    e_map, (rot_map, cen_map) = mean_reprojection_error(ctx, rec), mc.pose_errors(rec, scene["poses"])
    print("mapper: %d images, %d points, mean reprojection error %.6f px, max rotation error %.6f deg, max centre error %.6f"
          % (len(rec.images), len(rec.points3D), e_map, rot_map, cen_map))
    print("known-pose pipeline: %d points, mean reprojection error %.6f px, max rotation error %.6f deg, max centre error %.6f"
          % (n_ref, e_ref, rot_ref, cen_ref))
    print("rounds:", [(r["candidates"], r["registered"], r["points"]) for r in summary["rounds"]], "kernel ms:", summary["kernel_ms"])
    assert e_map <= 1.05 * e_ref
    assert rot_map <= 2.0 * rot_ref and cen_map <= 2.0 * cen_ref


def test_scene_a_registers_all_images(ctx):
    rec, summary = _map(ctx, "A")
    assert summary["status"] == "ok" and summary["num_reg_images"] == 10 and summary["unregistered"] == []
    assert len(rec.images) == 10 and len(rec.points3D) > 250
    _check_against_known_poses(ctx, "A", rec, summary)


def test_intrinsics_stay_unless_asked(ctx):
    """Default: the camera comes back as it went in.  With ba_refine_focal_length only the focal length moves, and stays where
    the data put it: 1800 observations with 0.5 px of noise over a field of about 500 px hold a focal length to far better
    than the 1 % asked here."""
    rec, _ = _map(ctx, "A")
    assert np.array_equal(rec.cameras[1].params, mc.PARAMS)
    rec, summary = _map(ctx, "A", {'ba_refine_focal_length': True})
    params = rec.cameras[1].params
    print("refined focal length %.4f (generated with %.1f)" % (params[0], mc.PARAMS[0]))
    assert summary["num_reg_images"] == 10
    assert params[0] != mc.PARAMS[0] and abs(params[0] - mc.PARAMS[0]) <= 0.01 * mc.PARAMS[0]
    assert np.array_equal(params[1:], mc.PARAMS[1:])


def test_scene_a_one_image_per_round(ctx):
    rec, summary = _map(ctx, "A", {'max_images_per_round': 1})
    assert summary["num_reg_images"] == 10 and all(r["registered"] <= 1 and r["candidates"] <= 1 for r in summary["rounds"])
    assert len(summary["rounds"]) == 9                                      # eight registrations and the round that finds nobody left
    _check_against_known_poses(ctx, "A", rec, summary)


def test_two_runs_give_identical_bits(ctx):
    a, sa = _map(ctx, "A")
    b, sb = _map(ctx, "A", fresh=True)
    assert sa["initial_pair"] == sb["initial_pair"] and sorted(a.images) == sorted(b.images) and sorted(a.points3D) == sorted(b.points3D)
    for i in a.images:
        assert np.array_equal(a.images[i].qvec, b.images[i].qvec) and np.array_equal(a.images[i].tvec, b.images[i].tvec)
    for p in a.points3D:
        assert np.array_equal(a.points3D[p].xyz, b.points3D[p].xyz)
        assert [(e.image_id, e.point2D_idx) for e in a.points3D[p].track.elements] == [(e.image_id, e.point2D_idx) for e in b.points3D[p].track.elements]


def test_hand_over_to_absolute_pose_without_a_host_copy(ctx):
    """pxr_absolute_pose on the visibility outputs as device pointers gives the bits of the same pairs uploaded from the host."""
    from pixsfm_amd.api.reconstruction import Image, Reconstruction
    from pixsfm_amd.api.triangulation import flatten_tracks
    from pixsfm_amd.engine import AbsolutePoseProblem, MapperScene, TriangulationProblem
    scene, _, _, graph, labels = _inputs("A")
    rec = Reconstruction()
    rec.add_camera(scene["camera"])
    for k, nm in enumerate(scene["names"]):
        rec.add_image(Image(k + 1, nm, 1, *scene["poses"][nm]))
    flat = flatten_tracks(rec, scene["keypoints"], graph, labels)
    d_xyz, d_status = TriangulationProblem(ctx, flat).triangulate()[:2]
    s = MapperScene(ctx, dict(flat, cam_size=np.array([[1000, 1000]], np.int32)))
    mask = np.ones(s.n_images, np.uint8)
    mask[3] = 0
    vis = s.visibility(d_xyz, d_status, mask, 6)
    n = vis["n_corr"]
    assert n > 1000
    on_device = AbsolutePoseProblem.from_device(ctx, vis["corr_offsets"], n, vis["corr_xy"], vis["corr_xyz"], s.d["image_camera"],
                                                s.d["cam_model"], s.d["cam_params"]).estimate()
    from_host = AbsolutePoseProblem(ctx, dict(query_offsets=vis["corr_offsets"].download(), xy=vis["corr_xy"].download()[:n],
                                              xyz=vis["corr_xyz"].download()[:n], query_camera=flat["image_camera"],
                                              cam_model=flat["cam_model"], cam_params=flat["cam_params"])).estimate()
    status = on_device[2].download()
    assert status[3] != 0 and (np.delete(status, 3) == 0).all()            # the masked-out image is a query without correspondences
    for a, b in zip(on_device, from_host):
        assert np.array_equal(a.download(), b.download(), equal_nan=True)


# ---- traps -------------------------------------------------------------------------------------------------------------------------
def test_unmatched_image_and_second_component_stay_unregistered(ctx):
    scene = _inputs("split")[0]
    rec, summary = _map(ctx, "split")
    assert summary["unregistered"] == scene["names"][10:]                  # the four images of the second ring, the image without matches
    assert summary["num_reg_images"] == 10 and sorted(im.name for im in rec.images.values()) == scene["names"][:10]
    assert set(summary["initial_pair"]) <= set(scene["names"][:10])


def _known_pose_share(ctx, kind):
    """The share of the tracks that the known-pose pipeline triangulates: the scene itself must be sound for a trap to mean
    anything.  Six-member tracks with noise of 0.5 px all triangulate under true poses; a wrong member in ten leaves a track at
    least four true members (0.9 of them would be enough: 0.8 asked)."""
    _, summary = _known_pose_pipeline(ctx, kind, None, refine=False)
    share = summary["status"]["ok"] / summary["num_tracks"]
    print("%s: the known-pose pipeline triangulates %.3f of %d tracks" % (kind, share, summary["num_tracks"]))
    return share


def test_cocentred_pair_is_not_the_initial_pair(ctx):
    scene, pairs, matches, _, _ = _inputs("cocentred")
    geoms = _geometries(ctx, "cocentred")
    twin = {scene["names"][0], scene["names"][-1]}
    p = [k for k, pr in enumerate(pairs) if set(pr) == twin][0]
    print("co-centred pair: success %s, inliers %s; most of the others: %d" %
          (geoms[p]["success"], geoms[p].get("num_inliers"), max(g.get("num_inliers", 0) for k, g in enumerate(geoms) if k != p)))
    assert geoms[p]["success"] and "config" not in geoms[p]
    assert geoms[p]["num_inliers"] == max(g.get("num_inliers", 0) for g in geoms)
    assert _known_pose_share(ctx, "cocentred") >= 0.8
    rec, summary = _map(ctx, "cocentred")
    print("initial pair trials:", summary["init_trials"])
    assert summary["init_trials"][0]["pair"] == pairs[p]                   # tried first, and turned down
    assert set(summary["initial_pair"]) != twin and summary["status"] == "ok"
    assert summary["num_reg_images"] == len(scene["names"])


def test_members_of_wrong_tracks_do_not_survive(ctx):
    scene = _inputs("wrong")[0]
    assert _known_pose_share(ctx, "wrong") >= 0.8
    rec, summary = _map(ctx, "wrong")
    assert summary["num_reg_images"] == 10 and summary["unregistered"] == []
    by_name = {im.name: im for im in rec.images.values()}
    n_wrong = 0
    for nm in scene["names"]:
        for f in np.flatnonzero(scene["wrong"][nm]):
            n_wrong += 1
            assert by_name[nm].points2D[f].point3D_id == -1, (nm, f)
    print("%d members of wrong tracks, none in a final track; %d points" % (n_wrong, len(rec.points3D)))
