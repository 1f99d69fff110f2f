"""Batched localization of queries against a map: the reference's second entry point, pixsfm/localize.py:main, without hloc.

The reference takes, per query, the database images retrieval returned, optionally splits them into covisibility clusters
(hloc.localize_sfm.do_covisibility_clustering), turns the query <-> database matches of every cluster into 2D-3D pairs
(hloc.localize_sfm.pose_from_cluster), localizes per cluster and keeps the cluster with the most inliers; its evaluation scripts
pick image pairs with hloc.pairs_from_covisibility (pixsfm/eval/eth3d/utils.py:73).  hloc is not installable where this library
runs; the three functions are restated in include/pixsfm_hip.h (pxr_covisibility, pxr_covisibility_clusters,
pxr_localization_pairs) as remembered -- PARITY WITH hloc IS NOT PINNED, the header is the specification.

`MapLocalizer.localize_queries` runs all queries at once: one matching launch over every (query, database image) pair, the
clusters kernel, one gather, one pxr_absolute_pose launch over every (query, cluster); the matches, the 2D-3D coordinates and the
poses' inputs never pass through the host.  `QueryLocalizer` (api.localization) stays what it is, and refines the winning
cluster per query when conf["refine"] holds one.
"""
import warnings
from copy import deepcopy

import numpy as np

from .. import _lib
from ..engine import AbsolutePoseProblem, CovisibilityGraph, LocalizationPairs, MatchProblem
from .keypoint_adjustment import default_context
from .localization import abspose_engine_options
from .matching import DescriptorMatcher
from .two_view import _camera_table


def map_arrays(reconstruction):
    """The flat arrays of a map: image_ids (ascending; the map image INDEX is the position in it), names, point_ids (ascending; the
    ROW of a point is the position in it), xyz (n_points, 3), the tracks of the points in CSR form over (track_offsets, obs_image)
    -- track elements in an image the map does not hold are left out -- and kp_point {image id: (n_keypoints,) int64, the row of
    the point a keypoint observes, -1 for none}."""
    rec = reconstruction
    image_ids = sorted(rec.images)
    index = {i: k for k, i in enumerate(image_ids)}
    point_ids = sorted(rec.points3D)
    row = {p: k for k, p in enumerate(point_ids)}
    offsets, obs_image = [0], []
    for p in point_ids:
        obs_image.extend(index[e.image_id] for e in rec.points3D[p].track.elements if e.image_id in index)
        offsets.append(len(obs_image))
    xyz = np.array([rec.points3D[p].xyz for p in point_ids], dtype=np.float64).reshape(-1, 3)
    kp_point = {i: np.array([row.get(int(p2.point3D_id), -1) for p2 in rec.images[i].points2D], dtype=np.int64) for i in image_ids}
    return dict(image_ids=image_ids, names=[rec.images[i].name for i in image_ids], point_ids=np.array(point_ids, np.int64), xyz=xyz,
                track_offsets=np.array(offsets, np.int64), obs_image=np.array(obs_image, np.int32), kp_point=kp_point)


def pairs_from_covisibility(reconstruction, num_matched, ctx=None):
    """hloc.pairs_from_covisibility: per map image, in ascending image id, its `num_matched` most covisible images as a list
    [(name, name)] -- the list DescriptorMatcher.match_pairs and unique_pairs take.  Covisibility of (i, j) = over the points i
    sees, the track elements in j (hloc's count); partners by (count descending, image id ascending) -- hloc leaves ties to
    argpartition, here they are defined; an image with fewer covisible partners gets fewer pairs.  Every call flattens the
    reconstruction (map_arrays) and counts again: keep the list, or an engine.CovisibilityGraph, when it is needed more than once."""
    m = map_arrays(reconstruction)
    if not m["image_ids"]:
        return []
    graph = CovisibilityGraph(ctx or default_context(), m["track_offsets"], m["obs_image"], len(m["image_ids"]))
    d_index, _, d_n = graph.topk(min(int(num_matched), _lib.MAX_COVIS_MATCHED))
    index, n = d_index.download(), d_n.download()
    return [(m["names"][i], m["names"][j]) for i in range(len(n)) for j in index[i, :n[i]]]


def covisibility_clustering(db_ids, reconstruction, ctx=None):
    """hloc.localize_sfm.do_covisibility_clustering for one query: the image ids `db_ids` (retrieval rank order) split into the
    connected components of covisibility among themselves, as a list of lists of image ids, largest first (of equal sizes, the
    one whose first member ranks first); inside a cluster the ids keep their rank order.  Runs the batched kernel on one list.
    Every call flattens the reconstruction and counts again; for many queries MapLocalizer (or engine.CovisibilityGraph.clusters
    over all lists at once) builds the counts once."""
    m = map_arrays(reconstruction)
    index = {i: k for k, i in enumerate(m["image_ids"])}
    db_ids = [int(i) for i in db_ids]
    for i in db_ids:
        if i not in index:
            raise KeyError("image id %d is not in the reconstruction" % i)
    if not db_ids:
        return []
    graph = CovisibilityGraph(ctx or default_context(), m["track_offsets"], m["obs_image"], len(m["image_ids"]))
    d_cluster, d_n = graph.clusters([0, len(db_ids)], [index[i] for i in db_ids])
    cluster, n = d_cluster.download(), int(d_n.download()[0])
    return [[i for i, c in zip(db_ids, cluster) if c == number] for number in range(n)]


# ---- the host side of localize_queries: plain functions of small arrays ---------------------------------------------------------
def retrieval_lists(retrieval, query_names):
    """{query: [db names in rank order]} from that dict or from the [(query, db)] list of pairs_from_retrieval; every name of
    query_names gets a list (an empty one when retrieval does not know it)."""
    if hasattr(retrieval, "items"):
        lists = {q: list(dbs) for q, dbs in retrieval.items()}
    else:
        lists = {}
        for q, db in retrieval:
            lists.setdefault(q, []).append(db)
    return {q: lists.get(q, []) for q in query_names}


def plan_batch(query_names, lists, map_index):
    """What one batch matches: names (the queries, then every database image some list names, in order of first appearance), db
    {query: the names of its list that the map holds -- the others are skipped with a warning, as pixsfm/localize.py:62-66 does},
    pairs (n_pairs, 2) int32 indices into names, (query, database image), the pairs of a query contiguous and in rank order,
    pair_first {query: its first pair}, ret_offsets (n_queries + 1) and ret (n_pairs,): the map image index of every pair's
    database image."""
    names, where = list(query_names), {q: k for k, q in enumerate(query_names)}
    queries = set(query_names)
    if len(queries) != len(names):
        raise ValueError("a query is named twice")
    db, pairs, ret, ret_offsets, pair_first = {}, [], [], [0], {}
    for q in query_names:
        kept = []
        for nm in lists[q]:
            if nm not in map_index:
                warnings.warn("Image %s was retrieved but not in database" % (nm,))
                continue
            kept.append(nm)
        if len(kept) > _lib.MAX_LOC_ENTRIES:
            raise ValueError("query %r has %d retrieved images, more than %d" % (q, len(kept), _lib.MAX_LOC_ENTRIES))
        db[q], pair_first[q] = kept, len(pairs)
        for nm in kept:
            if nm in queries:
                raise ValueError("image %r is both a query and a retrieved database image" % (nm,))
            if nm not in where:
                where[nm] = len(names)
                names.append(nm)
            pairs.append((where[q], where[nm]))
            ret.append(map_index[nm])
        ret_offsets.append(len(pairs))
    return dict(names=names, db=db, pairs=np.array(pairs, np.int32).reshape(-1, 2), pair_first=pair_first,
                ret_offsets=np.array(ret_offsets, np.int64), ret=np.array(ret, np.int32))


def problems_of(plan, cluster=None, n_clusters=None):
    """The problems of a batch: one per (query, cluster) in query order and cluster number, or with cluster None one per query
    with a list.  cluster (n_pairs,), n_clusters (n_queries,): what the clusters kernel wrote.  Returns problem_offsets,
    problem_pair (the pairs of a problem in rank order), problem_query and problem_cluster (per problem)."""
    off = plan["ret_offsets"]
    offsets, entries, p_query, p_cluster = [0], [], [], []
    for q in range(len(off) - 1):
        lo, hi = int(off[q]), int(off[q + 1])
        count = (1 if hi > lo else 0) if cluster is None else int(n_clusters[q])
        for c in range(count):
            entries.extend(e for e in range(lo, hi) if cluster is None or cluster[e] == c)
            offsets.append(len(entries))
            p_query.append(q)
            p_cluster.append(c)
    return dict(problem_offsets=np.array(offsets, np.int64), problem_pair=np.array(entries, np.int32),
                problem_query=np.array(p_query, np.int32), problem_cluster=np.array(p_cluster, np.int32))


def best_problems(n_queries, problem_query, status, n_inliers):
    """Per query the problem with the most inliers among those of status 0, ties to the lower cluster number (the earlier
    problem); -1 for a query whose every problem failed or that has none."""
    best = np.full(n_queries, -1, np.int64)
    for p, q in enumerate(problem_query):
        if status[p] == 0 and (best[q] < 0 or n_inliers[p] > n_inliers[best[q]]):
            best[q] = p
    return best


def collect_results(query_names, plan, problems, out, map_poses, point_ids):
    """The result of every query from the downloaded kernel outputs `out`: status, n_inliers (per problem), qvec, tvec (per
    problem), inlier (per correspondence), corr_offsets, corr_kp, corr_point (rows of the map's points).  map_poses {name: (qvec,
    tvec)}: a query whose every problem fails gets success False and the pose of its first retrieved image
    (pixsfm/localize.py:97-98; None, None without one)."""
    best = best_problems(len(query_names), problems["problem_query"], out["status"], out["n_inliers"])
    po, pp = problems["problem_offsets"], problems["problem_pair"]
    results = {}
    for q, name in enumerate(query_names):
        mine = np.flatnonzero(problems["problem_query"] == q)
        clusters = [[plan["names"][plan["pairs"][e, 1]] for e in pp[po[p]:po[p + 1]]] for p in mine]
        res = {"db": list(plan["db"][name]), "clusters": clusters}
        p = int(best[q])
        if p >= 0:
            lo, hi = int(out["corr_offsets"][p]), int(out["corr_offsets"][p + 1])
            res.update(success=True, qvec=np.array(out["qvec"][p]), tvec=np.array(out["tvec"][p]), num_inliers=int(out["n_inliers"][p]),
                       inliers=[bool(x) for x in out["inlier"][lo:hi]], best_cluster=int(problems["problem_cluster"][p]),
                       point2D_idxs=np.asarray(out["corr_kp"][lo:hi], dtype=np.int64),
                       point3D_ids=np.asarray(point_ids, dtype=np.int64)[np.asarray(out["corr_point"][lo:hi], dtype=np.int64)])
        else:
            qvec, tvec = map_poses[plan["db"][name][0]] if plan["db"][name] else (None, None)
            res.update(success=False, qvec=None if qvec is None else np.array(qvec, dtype=np.float64),
                       tvec=None if tvec is None else np.array(tvec, dtype=np.float64), num_inliers=0, inliers=[], best_cluster=-1,
                       point2D_idxs=np.zeros(0, np.int64), point3D_ids=np.zeros(0, np.int64))
        results[name] = res
    return results


def refine_results(results, refine, query_cameras, keypoints, query_fmaps=None, batch=False):
    """conf["refine"]: for every localized query, refine.localize(keypoints (n, 2), point2D_idxs, point3D_ids, camera,
    query_fmaps=query_fmaps[query] or None) on the winning problem's 2D-3D pairs -- QueryLocalizer.localize's arguments, unchanged.
    Where it succeeds, its qvec, tvec, num_inliers and inliers replace the batch's; point2D_idxs / point3D_ids stay, so `inliers`
    must be a mask over the pairs it was given, in their order, which is what QueryLocalizer.localize returns.  Where it fails the
    batch's pose stays.  In place.
    batch (conf["refine_batch"]) with a `refine` that has localize_batch: ONE refine.localize_batch call over the localized queries,
    with the same arguments per query, instead of the loop."""
    todo = [q for q, res in results.items() if res["success"]]
    args = [(np.asarray(keypoints[q], dtype=np.float64)[:, :2], list(results[q]["point2D_idxs"]), list(results[q]["point3D_ids"]),
             query_cameras[q]) for q in todo]
    fmaps = [None if query_fmaps is None else query_fmaps[q] for q in todo]
    if batch and hasattr(refine, "localize_batch"):
        fines = refine.localize_batch([dict(keypoints=a[0], pnp_point2D_idxs=a[1], pnp_points3D_id=a[2], query_camera=a[3], query_fmaps=f)
                                       for a, f in zip(args, fmaps)]) if todo else []
    else:
        fines = (refine.localize(*a, query_fmaps=f) for a, f in zip(args, fmaps))
    for q, fine in zip(todo, fines):
        res = results[q]
        if fine.get("success"):
            if len(fine["inliers"]) != len(res["point2D_idxs"]):
                raise ValueError("refine.localize returned %d inlier flags for the %d pairs of %r" % (len(fine["inliers"]), len(res["point2D_idxs"]), q))
            res.update({k: fine[k] for k in ("qvec", "tvec", "num_inliers", "inliers")})
    return results


class MapLocalizer:
    """pixsfm/localize.py:main for a batch of queries (module docstring).  The map's flat arrays -- tracks from points3D, the
    point of every keypoint from points2D[*].point3D_id, the points -- are built once here; the device copy of the points on the
    first localize_queries, and with it, once, the covisibility counts when conf["covisibility_clustering"] is set.  At most _lib.MAX_COVIS_IMAGES map images, _lib.MAX_LOC_ENTRIES retrieved
    images per query.

    conf: "matcher": a DescriptorMatcher conf (name or dict); "pnp": the options absolute_pose_estimation takes
    ("estimation_options", "refinement_options"; max_error 12 px as in the reference); "covisibility_clustering": localize per
    covisibility cluster of the retrieved images and keep the best (False, as in the reference); "refine": None, or a
    QueryLocalizer that is called per query, unchanged, on the winning cluster's 2D-3D pairs (QKA / QBA); "refine_batch": False,
    or True to refine all localized queries in one refine.localize_batch call (batched QKA, PnP and QBA launches) when `refine` has
    that method."""

    default_conf = {
        "matcher": "NN-mutual",
        "pnp": {"estimation_options": {"ransac": {"max_error": 12}}, "refinement_options": {}},
        "covisibility_clustering": False,
        "refine": None,
        "refine_batch": False,
    }

    def __init__(self, reconstruction, conf=None, ctx=None):
        conf = dict(conf or {})
        unknown = set(conf) - set(self.default_conf)
        if unknown:
            raise ValueError("unknown configuration key(s) %s" % sorted(unknown))
        self.conf = {**deepcopy({k: v for k, v in self.default_conf.items() if k != "refine"}), "refine": None, **conf}
        pnp = dict(self.conf["pnp"] or {})
        extra = set(pnp) - {"estimation_options", "refinement_options"}
        if extra:
            raise ValueError("unknown configuration key(s) %s in pnp" % sorted(extra))
        est = deepcopy(pnp.get("estimation_options") or {})
        est["ransac"] = {"max_error": 12, **(est.get("ransac") or {})}
        self.pnp_options = abspose_engine_options(est, pnp.get("refinement_options"))
        self.matcher = DescriptorMatcher.create(self.conf["matcher"])
        self.reconstruction = reconstruction
        self.ctx = ctx
        self.map = map_arrays(reconstruction)
        if len(self.map["image_ids"]) > _lib.MAX_COVIS_IMAGES:
            raise ValueError("%d map images, more than %d: the covisibility matrix is dense" % (len(self.map["image_ids"]), _lib.MAX_COVIS_IMAGES))
        self.map_index = {nm: k for k, nm in enumerate(self.map["names"])}
        self.map_poses = {reconstruction.images[i].name: (reconstruction.images[i].qvec, reconstruction.images[i].tvec) for i in self.map["image_ids"]}
        self.graph = self.d_xyz = None
        self.kernel_ms = None

    def _device(self):
        if self.d_xyz is None:
            self.ctx = self.ctx or default_context()
            self.d_xyz = self.ctx.to_device(self.map["xyz"], np.float64)
            if self.conf["covisibility_clustering"]:
                self.graph = CovisibilityGraph(self.ctx, self.map["track_offsets"], self.map["obs_image"], len(self.map["image_ids"]))
        return self.ctx

    def localize_queries(self, query_cameras, keypoints, descriptors, retrieval, query_fmaps=None, timed=False):
        """query_cameras {query name: Camera}; keypoints {name: (n, >= 2)} and descriptors {name: (n, D) float32, L2-normalised}
        for the queries and the database images (a database image's rows are its points2D); retrieval {query: [db names in rank
        order]} or the [(query, db)] list of pairs_from_retrieval.  query_fmaps {query: what QueryLocalizer.localize takes}: only
        for conf["refine"].  Returns {query: {"success", "qvec", "tvec", "num_inliers", "inliers", "best_cluster", "clusters",
        "db", "point2D_idxs", "point3D_ids"}} for every query of query_cameras: db = the retrieved names the map holds, clusters =
        their names per cluster number (one cluster without clustering), best_cluster = the cluster with the most inliers among
        those with a pose (ties: the lower number), point2D_idxs / point3D_ids / inliers = that cluster's 2D-3D pairs, ascending
        by query keypoint.  A query without a pose: success False, the pose of its first retrieved image, best_cluster -1.
        timed: keeps the kernels' times of every stage in self.kernel_ms {"match", "clusters", "pairs", "pnp"}."""
        query_names = list(query_cameras)
        plan = plan_batch(query_names, retrieval_lists(retrieval, query_names), self.map_index)
        names, n_q = plan["names"], len(query_names)
        for nm in names:
            if nm not in descriptors or nm not in keypoints:
                raise KeyError("no descriptors or keypoints for image %r" % (nm,))
        if len(plan["pairs"]) == 0:
            return collect_results(query_names, plan, problems_of(plan), dict(status=[], n_inliers=[]), self.map_poses, self.map["point_ids"])
        ctx = self._device()
        desc = [np.ascontiguousarray(descriptors[nm], dtype=np.float32) for nm in names]
        xy, kp_point = [], []
        for k, (nm, d) in enumerate(zip(names, desc)):
            kps = np.asarray(keypoints[nm], dtype=np.float64)
            kps = kps.reshape(0, 2) if kps.size == 0 else kps[:, :2]
            own = np.full(len(d), -1, np.int64) if k < n_q else self.map["kp_point"][self.map["image_ids"][self.map_index[nm]]]
            if d.ndim != 2 or len(kps) != len(d) or len(own) != len(d):
                raise ValueError("image %r: %s descriptors, %d keypoints, %d points2D in the map -- one row each" % (nm, d.shape, len(kps), len(own)))
            xy.append(kps)
            kp_point.append(own)
        ms = {}
        # 1. one matching launch over every (query, database image); matches0 stays on the device
        match = MatchProblem(ctx, desc, plan["pairs"])
        d_matches0, _, _ = match.run(timed=timed, **self.matcher.options())
        ms["match"] = match.kernel_ms
        # 2. the clusters of every query's list
        cluster = n_clusters = None
        if self.conf["covisibility_clustering"]:
            d_cluster, d_n = self.graph.clusters(plan["ret_offsets"], plan["ret"], timed=timed)
            cluster, n_clusters = d_cluster.download(), d_n.download()
            ms["clusters"] = self.graph.kernel_ms
        problems = problems_of(plan, cluster, n_clusters)
        # 3. one gather: the arguments of pxr_absolute_pose, on the device
        gather = LocalizationPairs(ctx, match, np.concatenate(xy), np.concatenate(kp_point), self.d_xyz)
        corr = gather.gather(d_matches0, problems["problem_offsets"], problems["problem_pair"], timed=timed)
        ms["pairs"] = gather.kernel_ms
        # 4. one absolute-pose launch over every problem
        cam_index, cam_model, cam_params = _camera_table([query_cameras[q] for q in query_names])
        pose = AbsolutePoseProblem.from_device(ctx, corr["corr_offsets"], corr["n_corr"], corr["corr_xy"], corr["corr_xyz"],
                                               ctx.to_device(cam_index[problems["problem_query"]], np.int32), ctx.to_device(cam_model, np.int32),
                                               ctx.to_device(cam_params, np.float64))
        d_q, d_t, d_status, d_ninl, _, d_inl, _ = pose.estimate(timed=timed, **self.pnp_options)
        ms["pnp"] = pose.kernel_ms
        self.kernel_ms = ms if timed else self.kernel_ms
        # 5. the best problem per query: a handful of numbers per problem, on the host
        n_corr = corr["n_corr"]
        out = dict(status=d_status.download(), n_inliers=d_ninl.download(), qvec=d_q.download(), tvec=d_t.download(),
                   inlier=d_inl.download()[:n_corr], corr_offsets=corr["corr_offsets"].download(),
                   corr_kp=corr["corr_kp"].download()[:n_corr], corr_point=corr["corr_point"].download()[:n_corr])
        results = collect_results(query_names, plan, problems, out, self.map_poses, self.map["point_ids"])
        if self.conf["refine"] is not None:
            refine_results(results, self.conf["refine"], query_cameras, keypoints, query_fmaps, batch=bool(self.conf["refine_batch"]))
        return results
