"""Batched map localization on the GPU: pxr_covisibility, pxr_covisibility_clusters and pxr_localization_pairs
(csrc/pxr_localize.hip) bit for bit against the numpy reference of tests/map_localization_cases.py on its boundary batch, twice with
the same bits; pairs_from_covisibility and covisibility_clustering on a map of two rings; MapLocalizer.localize_queries end to end
on that map, and the gather's outputs handed to pxr_absolute_pose where they are.

Bound of the end-to-end test (set by the issue that introduced the stage): the pose errors of the batched path against ground truth
may be twice what the existing per-query path (DescriptorMatcher.match_pairs, pairs_2d3d_from_matches, absolute_pose_estimation)
reaches for the same query on the same scene, both measured in the test -- the correspondences are the same set in another order, so the hash
sampling draws other samples and both routes end near the same minimum.  Measured on the MI355X: DESIGN.md section 32."""
import warnings

import numpy as np
import pytest

import map_localization_cases as lc

pytestmark = pytest.mark.gpu

PAIR_OUTPUTS = ("corr_kp", "corr_point", "corr_xy", "corr_xyz")


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(lc.COVIS_IMAGES)))
def test_covisibility_matches_the_reference_bit_for_bit(ctx, which):
    from pixsfm_amd.engine import CovisibilityGraph
    c = lc.boundary_batch()["covis"][which]
    graph = CovisibilityGraph(ctx, c["track_offsets"], c["obs_image"], c["n_images"], c["track_mask"], timed=True)
    assert np.array_equal(graph.counts(), c["count"])
    assert set(graph.kernel_ms) == {"check", "count", "topk"}
    for K in lc.NUM_MATCHED:
        runs = [[a.download() for a in graph.topk(K)] for _ in range(2)]
        for got, again, ref in zip(runs[0], runs[1], c["topk"][K]):
            assert np.array_equal(got, ref) and np.array_equal(got, again), K
        assert np.array_equal(graph.counts(), c["count"])


def _cluster_graph(ctx, count):
    """A CovisibilityGraph that holds a given count matrix (the boundary batch's is made by hand)."""
    from pixsfm_amd.engine import CovisibilityGraph
    graph = CovisibilityGraph(ctx, [0], [], len(count))
    graph.d_count.upload(count)
    return graph


def test_clusters_match_the_reference_bit_for_bit(ctx):
    k = lc.boundary_batch()["clusters"]
    graph = _cluster_graph(ctx, k["count"])
    runs = [[a.download() for a in graph.clusters(k["ret_offsets"], k["ret"], timed=True)] for _ in range(2)]
    for got, again, ref in zip(runs[0], runs[1], (k["cluster"], k["n_clusters"])):
        assert np.array_equal(got, ref) and np.array_equal(got, again)
    assert set(graph.kernel_ms) == {"check", "clusters"}


def _pairs_on_device(ctx, b):
    from pixsfm_amd.engine import LocalizationPairs, MatchProblem
    sizes = np.diff(b["image_offsets"])
    match = MatchProblem(ctx, [np.zeros((n, 4), np.float32) for n in sizes], b["pairs"])      # the matches are the batch's own
    assert np.array_equal(match.pair_offsets, b["pair_offsets"])
    return match, LocalizationPairs(ctx, match, b["kp_xy"], b["kp_point"], b["xyz"]), ctx.to_device(b["matches0"], np.int32)


def _sentinels(ctx, b, problem_pair):
    cap = int(np.diff(b["pair_offsets"])[np.clip(problem_pair, 0, len(b["pairs"]) - 1)].sum())
    n_p = len(b["problem_offsets"]) - 1
    return dict(corr_offsets=ctx.to_device(np.full(n_p + 1, -9, np.int64)), corr_kp=ctx.to_device(np.full(cap, -9, np.int32)),
                corr_point=ctx.to_device(np.full(cap, -9, np.int64)), corr_xy=ctx.to_device(np.full((cap, 2), -9.0)),
                corr_xyz=ctx.to_device(np.full((cap, 3), -9.0)))


def test_pairs_match_the_reference_bit_for_bit(ctx):
    pb = lc.boundary_batch()["pairs"]
    b, ref = pb["batch"], pb["ref"]
    match, gather, d_m = _pairs_on_device(ctx, b)
    runs = []
    for _ in range(2):
        got = gather.gather(d_m, b["problem_offsets"], b["problem_pair"], timed=True, out=_sentinels(ctx, b, b["problem_pair"]))
        assert got["n_corr"] == ref["n_corr"]
        runs.append({k: got[k].download() for k in PAIR_OUTPUTS + ("corr_offsets",)})
    assert set(gather.kernel_ms) == {"count", "scan", "write"}
    assert np.array_equal(runs[0]["corr_offsets"], ref["corr_offsets"])
    for k in PAIR_OUTPUTS:
        assert np.array_equal(runs[0][k][:ref["n_corr"]], ref[k]), k
        assert (runs[0][k][ref["n_corr"]:] == -9).all(), k + ": written past n_corr"
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(ctx):
    from pixsfm_amd._lib import PixsfmHipError
    from pixsfm_amd.engine import CovisibilityGraph
    bb = lc.boundary_batch()
    c = bb["covis"][-1]
    for name, replace, word in lc.bad_covisibility(c):
        if not set(replace) <= {"track_offsets", "obs_image"}:
            continue                                                                      # the limits are the Python layer's to refuse first
        with pytest.raises(PixsfmHipError, match=word):
            CovisibilityGraph(ctx, replace.get("track_offsets", c["track_offsets"]), replace.get("obs_image", c["obs_image"]), c["n_images"])
    k = bb["clusters"]
    graph = _cluster_graph(ctx, k["count"])
    for name, replace, word in lc.bad_clusters(k):
        if "n_images" in replace:
            graph.n_images = replace["n_images"]                                          # refused before the matrix is read
        with pytest.raises(PixsfmHipError, match=word):
            graph.clusters(replace.get("ret_offsets", k["ret_offsets"]), replace.get("ret", k["ret"]))
    b = bb["pairs"]["batch"]
    match, gather, d_m = _pairs_on_device(ctx, b)
    for name, replace, word in lc.bad_pairs(b):
        if not set(replace) <= {"problem_offsets", "problem_pair", "matches0"}:
            continue                                                                      # (the other arrays belong to the MatchProblem)
        entries = replace.get("problem_pair", b["problem_pair"])
        out = _sentinels(ctx, b, entries)
        d_bad = ctx.to_device(replace["matches0"], np.int32) if "matches0" in replace else d_m
        with pytest.raises(PixsfmHipError, match=word):
            gather.gather(d_bad, replace.get("problem_offsets", b["problem_offsets"]), entries, out=out)
        assert all((a.download() == -9).all() for a in out.values()), name


# ---- the host interface ----------------------------------------------------------------------------------------------------------
def test_pairs_from_covisibility_and_clustering_on_a_map_of_two_rings(ctx):
    from pixsfm_amd.api import covisibility_clustering, map_localization, pairs_from_covisibility
    tp = lc.two_places()
    rec = tp["reconstruction"]
    m = map_localization.map_arrays(rec)
    count = lc.covisibility_reference(m["track_offsets"], m["obs_image"], len(m["names"]))
    assert count.max() > 10 and (count[:6, 6:] == 0).all()                                # two places that share nothing
    for K in (1, 3, 20):
        index, _, n = lc.topk_reference(count, K)
        expected = [(m["names"][i], m["names"][j]) for i in range(len(n)) for j in index[i, :n[i]]]
        assert pairs_from_covisibility(rec, K, ctx=ctx) == expected
        assert len(expected) == (len(m["names"]) * K if K < 4 else int((count > 0).sum()))
    ids = m["image_ids"]
    mixed = [ids[k] for k in (7, 0, 8, 2, 1, 9, 3, 0)]                                    # both places interleaved, one image twice
    expected = [[mixed[e] for e in members] for members in lc.clusters_of_list(count, [ids.index(i) for i in mixed])]
    assert covisibility_clustering(mixed, rec, ctx=ctx) == expected
    assert [sorted(set(c)) for c in expected] == [sorted({ids[0], ids[1], ids[2], ids[3]}), sorted({ids[7], ids[8], ids[9]})]
    assert covisibility_clustering([], rec, ctx=ctx) == []


def _pose_error(qvec, tvec, truth):
    from pixsfm_amd import synthetic
    R, Rt = synthetic.qvec_to_rotmat(qvec), synthetic.qvec_to_rotmat(truth[0])
    rot = np.degrees(np.arccos(np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)))
    return float(rot), float(np.linalg.norm(-R.T @ tvec + Rt.T @ truth[1]))


MATCHER = {"distance_threshold": 0.7}      # true matches have distance 0, random unit descriptors about 1.4


def _per_query_path(ctx, tp):
    """The existing route: match one query against its list, pairs_2d3d_from_matches, absolute_pose_estimation."""
    from pixsfm_amd.api import DescriptorMatcher, absolute_pose_estimation, pairs_2d3d_from_matches
    rec, scene = tp["reconstruction"], tp["scene"]
    by_name = {im.name: im for im in rec.images.values()}
    out = {}
    for q in tp["queries"]:
        pairs = [(q, db) for db in tp["retrieval"][q]]
        matches, _ = DescriptorMatcher.create(MATCHER, ctx=ctx).match_pairs(tp["descriptors"], pairs)
        ids = {db: np.array([p.point3D_id for p in by_name[db].points2D]) for _, db in pairs}
        p2d, p3d = pairs_2d3d_from_matches([(db, m) for (_, db), m in zip(pairs, matches)], ids)
        res = absolute_pose_estimation(scene["keypoints"][q][p2d], [rec.points3D[i].xyz for i in p3d], scene["camera"],
                                       estimation_options={"ransac": {"max_error": 12}}, ctx=ctx)
        out[q] = dict(res, pairs=set(zip(p2d.tolist(), p3d.tolist())))
    return out


def test_localize_queries_end_to_end_on_a_map_of_two_places(ctx, monkeypatch):
    from pixsfm_amd import engine
    from pixsfm_amd.api import MapLocalizer, map_localization
    tp = lc.two_places()
    rec, scene, queries = tp["reconstruction"], tp["scene"], tp["queries"]
    assert len(queries) == 4 and len(rec.images) == 10 and max(len(v) for v in tp["retrieval"].values()) <= 16
    cameras = {q: scene["camera"] for q in queries}

    # every device-to-host copy the Python layer makes goes through pxr_memcpy_d2h: its source ranges are recorded
    handed, copied = [], []
    from_device, d2h = engine.AbsolutePoseProblem.from_device, ctx.lib.pxr_memcpy_d2h
    address = lambda p: int(getattr(p, "value", p) or 0)                                 # noqa: E731
    monkeypatch.setattr(map_localization.AbsolutePoseProblem, "from_device",
                        classmethod(lambda cls, c, off, n, xy, xyz, *rest: handed.append((xy, xyz, len(copied))) or from_device(c, off, n, xy, xyz, *rest)))
    monkeypatch.setattr(ctx.lib, "pxr_memcpy_d2h", lambda h, dst, src, n: copied.append((address(src), int(n))) or d2h(h, dst, src, n))

    reference = _per_query_path(ctx, tp)
    results = {}
    for clustering in (False, True):
        loc = MapLocalizer(rec, {"matcher": MATCHER, "covisibility_clustering": clustering}, ctx=ctx)
        results[clustering] = loc.localize_queries(cameras, scene["keypoints"], tp["descriptors"], tp["retrieval"], timed=True)
        assert set(loc.kernel_ms) >= {"match", "pairs", "pnp"}
    # the gather's coordinates went into pxr_absolute_pose where they were: device arrays out of which no byte was copied to the
    # host afterwards (they are alive since, so their addresses are theirs; the gather itself, before, copies nothing in Python)
    assert len(handed) == 2 and len(copied) > 10
    for xy, xyz, since in handed:
        assert len(copied) > since
        for a in (xy, xyz):
            assert isinstance(a, engine.DeviceArray)
            lo, hi = address(a.ptr), address(a.ptr) + max(a.nbytes, 1)
            assert lo and not any(src < hi and src + n > lo for src, n in copied[since:])

    for q in queries:
        assert reference[q]["success"], q                                                 # the scene is one the existing path localizes
        ref_rot, ref_centre = _pose_error(reference[q]["qvec"], reference[q]["tvec"], scene["poses"][q])
        print("%s per-query path: rotation error %.3e deg, centre error %.3e" % (q, ref_rot, ref_centre))
        whole, best = results[False][q], results[True][q]
        place = tp["place"][q]
        for name, res in (("whole list", whole), ("clusters", best)):
            rot, centre = _pose_error(res["qvec"], res["tvec"], scene["poses"][q]) if res["success"] else (np.inf, np.inf)
            print("%s %s: rotation error %.3e deg, centre error %.3e, %d inliers of %d (per-query path: %d)"
                  % (q, name, rot, centre, res["num_inliers"], len(res["inliers"]), reference[q]["num_inliers"]))
        for name, res in (("whole list", whole), ("clusters", best)):
            assert res["success"], (q, name)
            rot, centre = _pose_error(res["qvec"], res["tvec"], scene["poses"][q])
            assert rot <= 2 * ref_rot and centre <= 2 * ref_centre, (q, name, rot, centre)       # twice this query's own figure
            assert res["db"] == tp["retrieval"][q] and sum(res["inliers"]) == res["num_inliers"]
        # the whole list gives the per-query path's pairs: the same set, keypoints ascending
        assert whole["best_cluster"] == 0 and whole["clusters"] == [tp["retrieval"][q]]
        assert set(zip(whole["point2D_idxs"].tolist(), whole["point3D_ids"].tolist())) == reference[q]["pairs"]
        assert whole["point2D_idxs"].tolist() == sorted(whole["point2D_idxs"].tolist())
        # with clustering: two clusters, the places; the best one is the query's own
        assert len(best["clusters"]) == 2 and sorted(map(len, best["clusters"])) == [4, 6]
        assert {tp["place"][nm] for nm in best["clusters"][best["best_cluster"]]} == {place}
        alone = MapLocalizer(rec, {"matcher": MATCHER}, ctx=ctx).localize_queries(
            {q: cameras[q]}, scene["keypoints"], tp["descriptors"], {q: best["clusters"][best["best_cluster"]]})[q]
        assert alone["success"] and alone["num_inliers"] == best["num_inliers"]
        assert np.array_equal(alone["qvec"], best["qvec"]) and np.array_equal(alone["tvec"], best["tvec"])


def test_a_query_nobody_can_localize_and_an_unknown_database_image(ctx):
    from pixsfm_amd.api import MapLocalizer
    tp = lc.two_places()
    rec, scene = tp["reconstruction"], tp["scene"]
    q, lost = tp["queries"][0], "lost.jpg"
    rng = np.random.default_rng(0)
    keypoints = dict(scene["keypoints"], **{lost: rng.uniform(0, 1000, (40, 2))})
    noise = rng.normal(size=(40, 32)).astype(np.float32)
    descriptors = dict(tp["descriptors"], **{lost: noise / np.linalg.norm(noise, axis=1, keepdims=True)})
    first = tp["retrieval"][q][0]
    retrieval = [(q, "gone.jpg")] + [(q, db) for db in tp["retrieval"][q]] + [(lost, first), (lost, tp["retrieval"][q][1])]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = MapLocalizer(rec, {"matcher": MATCHER, "covisibility_clustering": True}, ctx=ctx).localize_queries(
            {q: scene["camera"], lost: scene["camera"]}, keypoints, descriptors, retrieval)
    assert any("gone.jpg" in str(x.message) for x in w)
    assert res[q]["success"] and res[q]["db"] == tp["retrieval"][q]
    truth = {im.name: im for im in rec.images.values()}[first]
    assert not res[lost]["success"] and res[lost]["num_inliers"] == 0 and res[lost]["best_cluster"] == -1
    assert np.array_equal(res[lost]["qvec"], truth.qvec) and np.array_equal(res[lost]["tvec"], truth.tvec)
