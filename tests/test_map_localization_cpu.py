"""Batched map localization without a GPU: the numpy reference of tests/map_localization_cases.py on hand-made cases whose answers
are written out here; the reference gather against api.matching.pairs_2d3d_from_matches; the source of the kernels
(csrc/pxr_localize.hip) run lane by lane over the stand-in runtime of tests/lane_emulation and held to the reference with exact
equality of every output on the boundary batch; every class of bad input, with outputs left untouched; and the host logic of
MapLocalizer.localize_queries on fabricated kernel outputs.  What only hardware can show (global atomics under contention, the
wavefront's real shuffles and ballots) stays with tests/test_map_localization_gpu.py."""
import ctypes as C
import warnings

import numpy as np
import pytest

import lanes
import map_localization_cases as lc
from lanes import p as _p


# ---- the reference on hand-made cases ----------------------------------------------------------------------------------------------
def test_a_track_seen_twice_by_one_image_counts_twice():
    # one track: image 0 twice, image 1 once, image 2 once
    count = lc.covisibility_reference([0, 4], [0, 1, 0, 2], 3)
    assert count.tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]
    # a second track (images 1, 2) that is masked out changes nothing, and counts when it is not
    assert lc.covisibility_reference([0, 4, 6], [0, 1, 0, 2, 1, 2], 3, [1, 0]).tolist() == count.tolist()
    assert lc.covisibility_reference([0, 4, 6], [0, 1, 0, 2, 1, 2], 3).tolist() == [[0, 2, 2], [2, 0, 2], [2, 2, 0]]


def test_count_ties_are_broken_by_index():
    count = np.array([[0, 3, 5, 3, 0], [3, 0, 0, 0, 0], [5, 0, 0, 0, 0], [3, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.int32)
    index, cnt, n = lc.topk_reference(count, 2)
    assert index.tolist() == [[2, 1], [0, -1], [0, -1], [0, -1], [-1, -1]]
    assert cnt.tolist() == [[5, 3], [3, 0], [5, 0], [3, 0], [0, 0]] and n.tolist() == [2, 1, 1, 1, 0]
    assert lc.topk_reference(count, 4)[0][0].tolist() == [2, 1, 3, -1]


def _chain_counts():
    """a - b - c (0 - 1 - 2) where a and c share nothing; 3 - 4 a pair apart; 5 alone"""
    count = np.zeros((6, 6), np.int32)
    for i, j in ((0, 1), (1, 2), (3, 4)):
        count[i, j] = count[j, i] = 1
    return count


def test_clusters_of_hand_made_lists():
    count = _chain_counts()
    assert lc.clusters_of_list(count, [0, 2, 1]) == [[0, 1, 2]]                          # the chain: one cluster
    assert lc.clusters_of_list(count, [0, 2]) == [[0], [1]]                              # without b: the walk stays inside the list
    assert lc.clusters_of_list(count, [3, 0, 1, 4]) == [[0, 3], [1, 2]]                  # equal sizes: ordered by first member
    assert lc.clusters_of_list(count, [5, 3, 0, 1, 4, 2]) == [[2, 3, 5], [1, 4], [0]]    # by size first
    assert lc.clusters_of_list(count, [5, 0, 5]) == [[0, 2], [1]]                        # an image listed twice: two connected entries
    cluster, n = lc.clusters_reference(count, [0, 3, 3, 7], [0, 2, 1, 3, 0, 1, 4])
    assert cluster.tolist() == [0, 0, 0, 0, 1, 1, 0] and n.tolist() == [1, 0, 2]


def test_reference_gather_agrees_with_pairs_2d3d_from_matches():
    """The same set of pairs and the same order within a keypoint, on the random problems of the boundary batch (keypoints
    ascend here, and appear in order of first appearance there)."""
    from pixsfm_amd.api import pairs_2d3d_from_matches
    b, ref = lc.boundary_batch()["pairs"]["batch"], lc.boundary_batch()["pairs"]["ref"]
    finite_point = np.isfinite(b["xyz"]).all(1)
    for p in range(len(b["problem_offsets"]) - 1):
        entries = b["problem_pair"][b["problem_offsets"][p]:b["problem_offsets"][p + 1]]
        items, ids = [], {}
        for j, pr in enumerate(entries):
            q, d = b["pairs"][pr]
            m = b["matches0"][b["pair_offsets"][pr]:b["pair_offsets"][pr + 1]]
            k = np.flatnonzero(m >= 0)
            k = k[np.isfinite(b["kp_xy"][b["image_offsets"][q] + k]).all(1)]              # what the host function is not asked about
            own = b["kp_point"][b["image_offsets"][d]:b["image_offsets"][d + 1]].copy()
            own[(own >= 0) & ~finite_point[np.maximum(own, 0)]] = -1
            items.append((j, np.stack([k, m[k]], 1)))
            ids[j] = own
        p2d, p3d = pairs_2d3d_from_matches(items, ids)
        lo, hi = ref["corr_offsets"][p], ref["corr_offsets"][p + 1]
        got = list(zip(ref["corr_kp"][lo:hi].tolist(), ref["corr_point"][lo:hi].tolist()))
        assert sorted(got) == sorted(zip(p2d.tolist(), p3d.tolist())), p
        for k in set(p2d.tolist()):
            assert [pid for kk, pid in got if kk == k] == p3d[p2d == k].tolist(), (p, k)
        assert ref["corr_kp"][lo:hi].tolist() == sorted(ref["corr_kp"][lo:hi].tolist())
    assert ref["n_corr"] > 100


def test_boundary_batch_holds_the_hand_made_keypoints():
    b, ref = lc.boundary_batch()["pairs"]["batch"], lc.boundary_batch()["pairs"]["ref"]
    lo, hi = ref["corr_offsets"][0], ref["corr_offsets"][1]                               # problem 0: all pairs of query 0
    of = lambda k: ref["corr_point"][lo:hi][ref["corr_kp"][lo:hi] == k].tolist()          # noqa: E731
    assert sorted(of(3)) == [7, 9] and of(4) == [] and of(5) == [] and of(6) == [] and of(8) == []
    assert ref["corr_offsets"][1] == ref["corr_offsets"][2] and ref["corr_offsets"][3] == ref["corr_offsets"][4]   # no entries; no keypoints
    c = lc.boundary_batch()["covis"][-1]
    assert c["count"].max() > 100 and (c["count"][-1] == 0).all() and (c["count"] == c["count"].T).all()
    assert (c["topk"][100][2] < 100).all() and c["topk"][100][2].max() > 1
    k = lc.boundary_batch()["clusters"]
    assert k["n_clusters"].tolist()[:2] == [0, 1] and k["n_clusters"][5:].tolist() == [1, 2, 2]


# ---- the kernels' source, lane by lane -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "localize_on_host.cpp")


def _raising(lib, rc, outputs):
    try:
        lanes.check(lib, rc)
    except ValueError as err:
        err.outputs = outputs
        raise
    return outputs


def run_covisibility(emu, c, partners, topk=True, **replace):
    lib, ctx = emu
    a = dict(track_offsets=c["track_offsets"], obs_image=c["obs_image"], track_mask=c["track_mask"], n_images=c["n_images"], num_matched=partners)
    a.update(replace)
    n, K = c["n_images"], max(partners, 1)
    out = dict(count=np.full((n, n), -9, np.int32), topk_index=np.full((n, K), -9, np.int32), topk_count=np.full((n, K), -9, np.int32),
               n_topk=np.full(n, -9, np.int32))
    off, img = np.ascontiguousarray(a["track_offsets"], np.int64), np.ascontiguousarray(a["obs_image"], np.int32)
    mask = None if a["track_mask"] is None else np.ascontiguousarray(a["track_mask"], np.uint8)
    rc = lib.pxr_covisibility(ctx, C.c_int32(a["n_images"]), C.c_int64(len(off) - 1), _p(off), C.c_int64(len(img)), _p(img), _p(mask),
                              C.c_int32(a["num_matched"]), _p(out["count"]), *((_p(out[k]) for k in ("topk_index", "topk_count", "n_topk")) if topk
                                                                               else (None, None, None)))
    return _raising(lib, rc, out)


def run_clusters(emu, k, **replace):
    lib, ctx = emu
    a = dict(count=k["count"], ret_offsets=k["ret_offsets"], ret=k["ret"])
    a.update(replace)
    count, off, ret = np.ascontiguousarray(a["count"], np.int32), np.ascontiguousarray(a["ret_offsets"], np.int64), np.ascontiguousarray(a["ret"], np.int32)
    out = dict(cluster=np.full(len(ret), -9, np.int32), n_clusters=np.full(len(off) - 1, -9, np.int32))
    rc = lib.pxr_covisibility_clusters(ctx, C.c_int32(a.get("n_images", len(count))), _p(count), C.c_int32(len(off) - 1), _p(off), C.c_int64(len(ret)), _p(ret),
                                       _p(out["cluster"]), _p(out["n_clusters"]))
    return _raising(lib, rc, out)


def run_pairs(emu, b, **replace):
    lib, ctx = emu
    a = dict(b)
    a.update(replace)
    types = dict(problem_offsets=np.int64, problem_pair=np.int32, pairs=np.int32, pair_offsets=np.int64, matches0=np.int32, image_offsets=np.int64,
                 kp_xy=np.float64, kp_point=np.int64, xyz=np.float64)
    a = {k: np.ascontiguousarray(a[k], t) for k, t in types.items()}
    n_p = len(a["problem_offsets"]) - 1
    rows = np.diff(b["pair_offsets"])
    cap = int(rows[np.clip(a["problem_pair"], 0, len(rows) - 1)].sum())                   # exactly what the header asks for
    out = dict(corr_offsets=np.full(n_p + 1, -9, np.int64), corr_kp=np.full(cap, -9, np.int32), corr_point=np.full(cap, -9, np.int64),
               corr_xy=np.full((cap, 2), -9.0), corr_xyz=np.full((cap, 3), -9.0))
    n_corr = C.c_int64(-9)
    rc = lib.pxr_localization_pairs(ctx, C.c_int32(n_p), _p(a["problem_offsets"]), C.c_int64(len(a["problem_pair"])), _p(a["problem_pair"]),
                                    C.c_int32(len(a["pairs"])), _p(a["pairs"]), _p(a["pair_offsets"]), C.c_int64(len(a["matches0"])), _p(a["matches0"]),
                                    C.c_int32(len(b["image_offsets"]) - 1), _p(a["image_offsets"]), C.c_int64(len(a["kp_xy"])), _p(a["kp_xy"]),
                                    _p(a["kp_point"]), C.c_int64(len(a["xyz"])), _p(a["xyz"]), _p(out["corr_offsets"]), _p(out["corr_kp"]),
                                    _p(out["corr_point"]), _p(out["corr_xy"]), _p(out["corr_xyz"]), C.byref(n_corr))
    out["n_corr"] = n_corr.value
    return _raising(lib, rc, out)


def equal_pairs(got, ref):
    n = ref["n_corr"]
    assert got["n_corr"] == n and np.array_equal(got["corr_offsets"], ref["corr_offsets"])
    for k in ("corr_kp", "corr_point", "corr_xy", "corr_xyz"):
        assert np.array_equal(np.asarray(got[k])[:n], ref[k]), k
        assert (np.asarray(got[k])[n:] == -9).all(), k + ": written past n_corr"


@pytest.mark.parametrize("which", range(len(lc.COVIS_IMAGES)))
def test_covisibility_source_matches_the_reference_on_the_boundary_batch(emu, which):
    c = lc.boundary_batch()["covis"][which]
    for K in lc.NUM_MATCHED:
        got = run_covisibility(emu, c, K)
        assert np.array_equal(got["count"], c["count"])
        for k, ref in zip(("topk_index", "topk_count", "n_topk"), c["topk"][K]):
            assert np.array_equal(got[k], ref), (k, K)
    got = run_covisibility(emu, c, 0, topk=False)                                         # counts alone: num_matched is ignored
    assert np.array_equal(got["count"], c["count"]) and (got["n_topk"] == -9).all()
    got = run_covisibility(emu, c, 1, track_mask=None)
    assert np.array_equal(got["count"], lc.covisibility_reference(c["track_offsets"], c["obs_image"], c["n_images"]))


def test_clusters_source_matches_the_reference_on_the_boundary_batch(emu):
    k = lc.boundary_batch()["clusters"]
    got = run_clusters(emu, k)
    assert np.array_equal(got["cluster"], k["cluster"]) and np.array_equal(got["n_clusters"], k["n_clusters"])
    c = lc.boundary_batch()["covis"][-1]                                                  # and on counts the other kernel would write
    ret_off, ret = np.array([0, 64, 70]), np.concatenate([np.arange(64, 0, -1), [64, 3, 64, 40, 3, 64]])
    got = run_clusters(emu, dict(count=c["count"], ret_offsets=ret_off, ret=ret))
    ref = lc.clusters_reference(c["count"], ret_off, ret)
    assert np.array_equal(got["cluster"], ref[0]) and np.array_equal(got["n_clusters"], ref[1])
    assert ref[1].min() >= 2                                                              # image 64 observes nothing: a cluster of its own


def test_pairs_source_matches_the_reference_on_the_boundary_batch(emu):
    pb = lc.boundary_batch()["pairs"]
    equal_pairs(run_pairs(emu, pb["batch"]), pb["ref"])


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(emu):
    bb = lc.boundary_batch()

    def refused(run, cases, *args):
        for name, replace, word in cases:
            with pytest.raises(ValueError, match=word) as e:
                run(emu, *args, **replace)
            assert e.value.args[0].startswith("-1:"), name                                # PXR_EINVAL
            assert all((np.asarray(v) == -9).all() for v in e.value.outputs.values()), name
    refused(run_covisibility, lc.bad_covisibility(bb["covis"][-1]), bb["covis"][-1], 4)
    refused(run_clusters, lc.bad_clusters(bb["clusters"]), bb["clusters"])
    refused(run_pairs, lc.bad_pairs(bb["pairs"]["batch"]), bb["pairs"]["batch"])


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: 17 images, tracks around the 16 lanes of a group, lists of 0, 1, 63 and 64
    entries, a problem of 64 entries."""
    stdout = lanes.sanitized(tmp_path, "localize_on_host.cpp", "LOCALIZE_ON_HOST_MAIN", 17, 1, 40, 2, 15, 16, 17, 33, 300, 0, 5)
    rows = {int(ln.split()[2]): [int(x) for x in ln.split()[4::2]] for ln in stdout.split("\n") if ln.startswith("covisibility K")}
    assert set(rows) == {1, 100} and rows[1][0] == rows[100][0] > 0 and rows[1][1:3] == [0, 0]        # symmetric, empty diagonal
    assert rows[1][3] <= 17 < rows[100][3] and rows[1][4] == rows[100][4]                            # partners; the best one's count
    clusters = [int(x) for x in [ln for ln in stdout.split("\n") if ln.startswith("clusters")][0].split()[1:]]
    assert clusters[:2] == [0, 1] and all(1 <= c <= 64 for c in clusters[2:])
    pairs = [ln for ln in stdout.split("\n") if ln.startswith("pairs")][0].split()
    offsets = [int(x) for x in pairs[6:]]
    assert offsets[0] == 0 and offsets[1] == offsets[2] == offsets[3] and offsets[-1] == int(pairs[4]) <= int(pairs[2])
    assert 0 < offsets[1] == offsets[4] - offsets[3] <= 3 * 70                                         # 64 entries over the same three pairs: the same set


# ---- the host logic of localize_queries --------------------------------------------------------------------------------------------
def _tiny_map():
    from pixsfm_amd.api.reconstruction import Camera, Image, Point2D, Point3D, Reconstruction, Track, TrackElement
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_PINHOLE", 640, 480, [500.0, 320.0, 240.0]))
    for i, nm in enumerate(["a", "b", "c", "d"], 1):
        rec.add_image(Image(i, nm, 1, [1.0, 0, 0, 0], [float(i), 0, 0], [Point2D([10.0 * k, 5.0], 100 + k if k < 2 else -1) for k in range(3)]))
    rec.add_point3D(100, Point3D([0, 0, 5.0], Track([TrackElement(1, 0), TrackElement(2, 0)])))      # a - b
    rec.add_point3D(101, Point3D([1, 0, 5.0], Track([TrackElement(3, 1), TrackElement(4, 1), TrackElement(9, 0)])))   # c - d (and an image the map lacks)
    return rec


def test_map_arrays_and_plan_skip_what_the_map_lacks():
    from pixsfm_amd.api import map_localization as ml
    m = ml.map_arrays(_tiny_map())
    assert m["names"] == ["a", "b", "c", "d"] and m["point_ids"].tolist() == [100, 101]
    assert m["track_offsets"].tolist() == [0, 2, 4] and m["obs_image"].tolist() == [0, 1, 2, 3]
    assert m["kp_point"][1].tolist() == [0, 1, -1]
    lists = ml.retrieval_lists([("q1", "c"), ("q1", "nowhere"), ("q1", "a"), ("q2", "b")], ["q1", "q2", "q3"])
    assert lists == {"q1": ["c", "nowhere", "a"], "q2": ["b"], "q3": []}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        plan = ml.plan_batch(["q1", "q2", "q3"], lists, {nm: k for k, nm in enumerate(m["names"])})
    assert len(w) == 1 and "nowhere" in str(w[0].message)
    assert plan["names"] == ["q1", "q2", "q3", "c", "a", "b"] and plan["db"] == {"q1": ["c", "a"], "q2": ["b"], "q3": []}
    assert plan["pairs"].tolist() == [[0, 3], [0, 4], [1, 5]] and plan["ret"].tolist() == [2, 0, 1] and plan["ret_offsets"].tolist() == [0, 2, 3, 3]
    with pytest.raises(ValueError, match="more than 64"):
        ml.plan_batch(["q"], {"q": ["a"] * 65}, {"a": 0})


def test_best_cluster_ties_and_the_fallback_pose():
    from pixsfm_amd.api import map_localization as ml
    rec = _tiny_map()
    loc = ml.MapLocalizer(rec, {"covisibility_clustering": True})                         # no device is touched before localize_queries
    lists = {"q1": ["c", "a", "d"], "q2": ["a", "c"], "q3": ["b"], "q4": []}
    names = list(lists)
    plan = ml.plan_batch(names, lists, loc.map_index)
    # as the clusters kernel would answer: q1 {c, d} | {a}; q2 {a} | {c}; q3 {b}
    cluster, n_clusters = np.array([0, 1, 0, 0, 1, 0]), np.array([2, 2, 1, 0])
    pr = ml.problems_of(plan, cluster, n_clusters)
    assert pr["problem_offsets"].tolist() == [0, 2, 3, 4, 5, 6] and pr["problem_pair"].tolist() == [0, 2, 1, 3, 4, 5]
    assert pr["problem_query"].tolist() == [0, 0, 1, 1, 2] and pr["problem_cluster"].tolist() == [0, 1, 0, 1, 0]
    whole = ml.problems_of(plan)
    assert whole["problem_offsets"].tolist() == [0, 3, 5, 6] and whole["problem_query"].tolist() == [0, 1, 2]
    # q1: cluster 1 has more inliers; q2: a tie, the lower number wins over a failed... and over an equal one; q3: its only problem fails
    status, n_inl = np.array([0, 0, 0, 0, 3]), np.array([5, 9, 7, 7, 0])
    assert ml.best_problems(4, pr["problem_query"], status, n_inl).tolist() == [1, 2, -1, -1]
    assert ml.best_problems(4, pr["problem_query"], np.array([0, 2, 0, 0, 3]), n_inl).tolist() == [0, 2, -1, -1]   # more inliers, but no pose
    corr_offsets = np.array([0, 2, 5, 6, 6, 6])
    out = dict(status=status, n_inliers=n_inl, qvec=np.tile([1.0, 0, 0, 0], (5, 1)), tvec=np.arange(15.0).reshape(5, 3),
               inlier=np.array([1, 0, 1, 1, 0, 1], np.uint8), corr_offsets=corr_offsets, corr_kp=np.array([0, 1, 0, 0, 2, 1]),
               corr_point=np.array([0, 1, 1, 0, 1, 1]))
    res = ml.collect_results(names, plan, pr, out, loc.map_poses, loc.map["point_ids"])
    assert res["q1"]["success"] and res["q1"]["best_cluster"] == 1 and res["q1"]["num_inliers"] == 9
    assert res["q1"]["clusters"] == [["c", "d"], ["a"]] and res["q1"]["db"] == ["c", "a", "d"]
    assert res["q1"]["point2D_idxs"].tolist() == [0, 0, 2] and res["q1"]["point3D_ids"].tolist() == [101, 100, 101]
    assert res["q1"]["inliers"] == [True, True, False] and res["q1"]["tvec"].tolist() == [3.0, 4.0, 5.0]
    assert res["q2"]["best_cluster"] == 0 and res["q2"]["point3D_ids"].tolist() == [101]
    assert not res["q3"]["success"] and res["q3"]["tvec"].tolist() == [2.0, 0, 0] and res["q3"]["best_cluster"] == -1   # image b's pose
    assert not res["q4"]["success"] and res["q4"]["qvec"] is None and res["q4"]["clusters"] == []
    with pytest.raises(ValueError, match="unknown"):
        ml.MapLocalizer(rec, {"clustering": True})


def test_refine_is_called_per_localized_query_and_merged():
    """conf["refine"] through a stand-in for QueryLocalizer: the arguments it gets and what is taken from its answer."""
    from pixsfm_amd.api import map_localization as ml
    calls = []

    class Stub:
        def localize(self, keypoints, point2D_idxs, point3D_ids, camera, query_fmaps=None):
            calls.append((keypoints, point2D_idxs, point3D_ids, camera, query_fmaps))
            if camera == "cam-b":
                return {"success": False}
            return {"success": True, "qvec": np.array([0.0, 1, 0, 0]), "tvec": np.array([7.0, 8, 9]), "num_inliers": 1, "inliers": [False, True],
                    "covariance": "not taken"}

    def result(success, tag):
        return dict(success=success, qvec=np.array([1.0, 0, 0, 0]), tvec=np.full(3, tag), num_inliers=2 if success else 0,
                    inliers=[True, True] if success else [], best_cluster=0 if success else -1, clusters=[["a"]], db=["a"],
                    point2D_idxs=np.array([4, 6] if success else [], np.int64), point3D_ids=np.array([100, 101] if success else [], np.int64))
    results = {"qa": result(True, 1.0), "qb": result(True, 2.0), "qc": result(False, 3.0)}
    keypoints = {q: np.arange(24.0).reshape(8, 3) + k for k, q in enumerate(results)}       # a third column (scale) is cut off
    out = ml.refine_results(results, Stub(), {"qa": "cam-a", "qb": "cam-b", "qc": "cam-c"}, keypoints, {"qa": "fm-a", "qb": "fm-b", "qc": "fm-c"})
    assert out is results and [c[3] for c in calls] == ["cam-a", "cam-b"]                    # not the query without a pose
    kp, idx, ids, cam, fmaps = calls[0]
    assert kp.shape == (8, 2) and np.array_equal(kp, keypoints["qa"][:, :2]) and idx == [4, 6] and ids == [100, 101] and fmaps == "fm-a"
    a = results["qa"]
    assert a["tvec"].tolist() == [7.0, 8, 9] and a["qvec"].tolist() == [0.0, 1, 0, 0] and a["num_inliers"] == 1 and a["inliers"] == [False, True]
    assert a["point2D_idxs"].tolist() == [4, 6] and a["best_cluster"] == 0 and "covariance" not in a
    assert results["qb"]["tvec"].tolist() == [2.0] * 3 and results["qb"]["num_inliers"] == 2    # the refinement failed: the batch's pose stays
    assert not results["qc"]["success"] and results["qc"]["tvec"].tolist() == [3.0] * 3
    ml.refine_results({"qa": result(True, 1.0)}, Stub(), {"qa": "cam-a"}, keypoints)            # without query_fmaps
    assert calls[-1][4] is None

    class Short(Stub):
        def localize(self, *args, **kwargs):
            return dict(Stub.localize(self, *args, **kwargs), inliers=[True])
    with pytest.raises(ValueError, match="inlier flags"):
        ml.refine_results({"qa": result(True, 1.0)}, Short(), {"qa": "cam-a"}, keypoints)


def test_entry_points_are_declared_and_exported():
    from pixsfm_amd import _lib, api, engine
    for name in ("pxr_covisibility", "pxr_covisibility_clusters", "pxr_localization_pairs"):
        assert name in _lib.declared_symbols() and name + "_timed" in _lib.declared_symbols()
    assert api.MapLocalizer and api.pairs_from_covisibility and api.covisibility_clustering
    assert engine.CovisibilityGraph and engine.LocalizationPairs
