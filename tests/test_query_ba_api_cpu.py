"""The Python layer of the batched query bundle adjustment without a GPU: the argument checks of QueryBundleOptimizer.run_batch,
QueryBundleAdjuster.refine_batch / refine_multilevel_batch and QueryLocalizer.localize_batch, the decision to fall back to run()
per query, and MapLocalizer's "refine_batch" key.  What runs on the device is tests/test_query_ba_gpu.py's."""
import numpy as np
import pytest


def _query(n=3, **change):
    q = dict(qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3), camera="cam", points3D=[np.zeros(3)] * n, fmap="fmap",
             references=[np.zeros((1, 128))] * n, inliers=None, patch_idxs=None)
    q.update(change)
    return tuple(q[k] for k in ("qvec", "tvec", "camera", "points3D", "fmap", "references", "inliers", "patch_idxs"))


@pytest.mark.parametrize("method", ["run_batch", "refine_batch"])
def test_run_batch_checks_what_run_checks_before_anything_runs(method):
    from pixsfm_amd.api.localization import QueryBundleAdjuster, QueryBundleOptimizer
    target = QueryBundleOptimizer() if method == "run_batch" else QueryBundleAdjuster()
    solver = target if method == "run_batch" else target.solver
    solver.run = lambda *a, **k: pytest.fail("a query ran although the batch is invalid")
    call = getattr(target, method)
    for bad, word in ((_query(references=[np.zeros((1, 128))] * 2), "references"), (_query(patch_idxs=[0, 1]), "patch_idxs"),
                      (_query(inliers=[True]), "inliers"), (_query(qvec=np.array([1.0, 0, 0, 0], np.float32)), "qvec"),
                      (_query(qvec=[1.0, 0, 0, 0]), "qvec"), (_query(tvec=np.zeros(4)), "tvec"), (_query()[:5], "a query is")):
        with pytest.raises(ValueError, match=word):
            call([_query(), bad])
    assert call([]) == []


def test_refine_multilevel_batch_wants_the_same_levels_everywhere():
    from pixsfm_amd.api.localization import QueryBundleAdjuster
    adj = QueryBundleAdjuster()
    seen = []
    adj.solver.run_batch = lambda queries: seen.append([(q[4], q[5]) for q in queries]) or [True] * len(queries)
    two = _query(fmap=["level 0", "level 1"], references=[["r0"], ["r1"]])
    assert adj.refine_multilevel_batch([two, two[:6]]) == [True, True]
    assert seen == [[("level 1", ["r1"])] * 2, [("level 0", ["r0"])] * 2]              # the last level first, as refine_multilevel
    with pytest.raises(ValueError, match="levels"):
        adj.refine_multilevel_batch([two, _query(fmap=["one"], references=[["r"]])])
    with pytest.raises(ValueError, match="levels"):
        adj.refine_multilevel_batch([_query(fmap=["a", "b"], references=[["r"]])])
    assert adj.refine_multilevel_batch([]) == []


def test_the_fall_back_decision():
    from pixsfm_amd.api.localization import QueryBundleOptimizer
    from pixsfm_amd.engine import query_ba_supported
    assert QueryBundleOptimizer().batch_fallback_reason() is None
    for key in ("refine_focal_length", "refine_principal_point", "refine_extra_params"):
        assert "intrinsics" in QueryBundleOptimizer({key: True}).batch_fallback_reason()
    assert "callbacks" in QueryBundleOptimizer({"solver": {"callbacks": [lambda s: 0]}}).batch_fallback_reason()

    class Arena:
        def __init__(self, dtype, C):
            self.dtype, self.C = dtype, C
    assert all(query_ba_supported(Arena(dt, ch)) for dt in (np.float16, np.float32, np.float64) for ch in (128, 64))
    assert not any(query_ba_supported(Arena(dt, ch)) for dt, ch in ((np.float16, 32), (np.float32, 3), (np.float64, 1), (np.uint8, 128)))

    # with a refine_* option every query goes through run(), with run()'s arguments, and its summary is kept
    opt = QueryBundleOptimizer({"refine_focal_length": True})
    calls = []

    def run(qvec, tvec, camera, points3D, fmap, references, inliers=None, patch_idxs=None):
        calls.append((camera, len(points3D), inliers, patch_idxs))
        opt.last_summary = {"final_cost": float(len(calls))}
        return len(points3D) > 0
    opt.run = run
    ok = opt.run_batch([_query(camera="a", inliers=[True, False, True]), _query(0, camera="b"), _query(2, camera="c", patch_idxs=[5, 6])[:8]])
    assert ok == [True, False, True] and opt.last_batch_path == "per_query" and "intrinsics" in opt.last_batch_reason
    assert calls == [("a", 3, [True, False, True], None), ("b", 0, None, None), ("c", 2, None, [5, 6])]
    assert opt.last_summaries == [{"final_cost": 1.0}, None, {"final_cost": 3.0}]


def _tiny_map():
    from pixsfm_amd.api.reconstruction import Camera, Image, Point2D, Point3D, Reconstruction, Track, TrackElement
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_PINHOLE", 640, 480, [500.0, 320.0, 240.0]))
    for i, nm in enumerate(["a", "b"], 1):
        rec.add_image(Image(i, nm, 1, [1.0, 0, 0, 0], [float(i), 0, 0], [Point2D([10.0 * k, 5.0], 100 + k if k < 2 else -1) for k in range(3)]))
    rec.add_point3D(100, Point3D([0, 0, 5.0], Track([TrackElement(1, 0), TrackElement(2, 0)])))
    rec.add_point3D(101, Point3D([1, 0, 5.0], Track([TrackElement(1, 1), TrackElement(2, 1)])))
    return rec


def test_localize_batch_checks_its_arguments():
    from pixsfm_amd.api.localization import QueryLocalizer
    rec = _tiny_map()
    cam = rec.cameras[1]
    loc = QueryLocalizer(rec, {}, references=[{}])
    kp = np.zeros((4, 2))
    good = dict(keypoints=kp, pnp_point2D_idxs=[0, 1], pnp_points3D_id=[100, 101], query_camera=cam, query_fmaps=["fm"])
    with pytest.raises(ValueError, match=r"return_covariance=True\) per query"):
        loc.localize_batch([dict(good, return_covariance=True)])
    with pytest.raises(ValueError, match=r"return_covariance=True\) per query"):
        loc.localize_batch([(kp, [0, 1], [100, 101], cam, None, ["fm"], True)])
    with pytest.raises(ValueError, match="same length"):
        loc.localize_batch([dict(good, pnp_points3D_id=[100])])
    with pytest.raises(ValueError, match="unknown argument"):
        loc.localize_batch([dict(good, fmaps=["fm"])])
    with pytest.raises(ValueError, match="needs 'query_camera'"):
        loc.localize_batch([{k: v for k, v in good.items() if k != "query_camera"}])
    with pytest.raises(ValueError, match="a query is"):
        loc.localize_batch([(kp, [0, 1], [100, 101])])
    with pytest.raises(ValueError, match="image_path or query_fmaps"):
        loc.localize_batch([dict(good, query_fmaps=None)])
    stacked = QueryLocalizer(rec, {"QKA": {"stack_correspondences": True}}, references=[{}])
    with pytest.raises(ValueError, match=r"call localize\(\) per query"):
        stacked.localize_batch([good])
    # queries without pairs are answered without a device, as localize() answers them
    none = dict(good, pnp_point2D_idxs=[], pnp_points3D_id=[])
    assert loc.localize_batch([none, (kp, [], [], cam)]) == [{"success": False}] * 2 == [loc.localize(kp, [], [], cam, query_fmaps=["fm"])] * 2
    assert loc.localize_batch([]) == []


def test_map_localizer_refine_batch_key():
    from pixsfm_amd.api import map_localization as ml
    rec = _tiny_map()
    assert ml.MapLocalizer.default_conf["refine_batch"] is False and ml.MapLocalizer(rec).conf["refine_batch"] is False
    assert ml.MapLocalizer(rec, {"refine_batch": True, "refine": "r"}).conf["refine_batch"] is True
    calls = []

    class Loop:
        def localize(self, keypoints, point2D_idxs, point3D_ids, camera, query_fmaps=None):
            calls.append(("localize", camera, query_fmaps))
            return {"success": True, "qvec": np.array([0.0, 1, 0, 0]), "tvec": np.full(3, 7.0), "num_inliers": 1, "inliers": [False, True]}

    class Batch(Loop):
        def localize_batch(self, queries):
            calls.append(("localize_batch", [(sorted(q), q["query_camera"], q["query_fmaps"], q["pnp_point2D_idxs"], q["pnp_points3D_id"],
                                              q["keypoints"].shape) for q in queries]))
            return [{"success": False} if q["query_camera"] == "cam-b" else Loop.localize(self, None, None, None, None) for q in queries]

    def results():
        def one(success, tag):
            return dict(success=success, qvec=np.array([1.0, 0, 0, 0]), tvec=np.full(3, tag), num_inliers=2 if success else 0,
                        inliers=[True, True] if success else [], point2D_idxs=np.array([4, 6] if success else [], np.int64),
                        point3D_ids=np.array([100, 101] if success else [], np.int64))
        return {"qa": one(True, 1.0), "qb": one(True, 2.0), "qc": one(False, 3.0)}
    cams, fmaps = {"qa": "cam-a", "qb": "cam-b", "qc": "cam-c"}, {"qa": "fm-a", "qb": "fm-b", "qc": "fm-c"}
    keypoints = {q: np.arange(24.0).reshape(8, 3) for q in cams}
    res = ml.refine_results(results(), Batch(), cams, keypoints, fmaps, batch=True)
    keys = sorted(["keypoints", "pnp_point2D_idxs", "pnp_points3D_id", "query_camera", "query_fmaps"])
    assert calls[0] == ("localize_batch", [(keys, "cam-a", "fm-a", [4, 6], [100, 101], (8, 2)), (keys, "cam-b", "fm-b", [4, 6], [100, 101], (8, 2))])
    assert [c[0] for c in calls] == ["localize_batch", "localize"]                            # one call; (the stub's own use of Loop.localize)
    assert res["qa"]["tvec"].tolist() == [7.0] * 3 and res["qa"]["inliers"] == [False, True] and res["qb"]["tvec"].tolist() == [2.0] * 3
    assert not res["qc"]["success"]
    # the default, and a refine without localize_batch: the loop
    for refine, batch in ((Batch(), False), (Loop(), True)):
        del calls[:]
        res = ml.refine_results(results(), refine, cams, keypoints, fmaps, batch=batch)
        assert calls == [("localize", "cam-a", "fm-a"), ("localize", "cam-b", "fm-b")] and res["qb"]["tvec"].tolist() == [7.0] * 3
    del calls[:]
    assert ml.refine_results({"qc": results()["qc"]}, Batch(), cams, keypoints, fmaps, batch=True)["qc"]["success"] is False and calls == []


def test_entry_points_are_declared_and_exported():
    from pixsfm_amd import _lib, engine
    from pixsfm_amd.api.localization import QueryBundleAdjuster, QueryBundleOptimizer, QueryLocalizer
    assert "pxr_query_ba_solve" in _lib.declared_symbols() and "pxr_query_ba_solve_timed" in _lib.declared_symbols()
    assert engine.QueryBAProblem and QueryBundleOptimizer.run_batch and QueryBundleAdjuster.refine_multilevel_batch and QueryLocalizer.localize_batch
