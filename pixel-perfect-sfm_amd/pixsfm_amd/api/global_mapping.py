"""Global mapping for the accelerated path: verified matches in, poses and points out, all images at once.

`GlobalMapper.create(conf).reconstruct(cameras, keypoints, graph, pairs, geometries)` takes what IncrementalMapper.reconstruct takes
and returns what it returns, so the two are interchangeable.  Where the incremental mapper grows a model from one initial pair,
this one solves for all rotations at once (pxr_rotation_averaging over the relative rotations of the verified pairs), then for all
camera centres and points at once (pxr_global_positioning over the observations' rays and the pairs' baseline directions), and
hands over to the stages the incremental mapper ends with: track triangulation, geometric bundle adjustment, the reprojection
filter.  It needs no initial pair and no registration order, so a low-parallax sequence on which no pair
passes the incremental mapper's initial-pair criteria still reconstructs.  It is deterministic and has no random state.  Parity
with COLMAP / GLOMAP is not pinned.  Out of scope: several models per scene, uncalibrated pairs (dropped), registering the images
outside the largest component, more than PXR_MAX_IMAGES_DIRECT + 1 = 1001 images.
"""
import time

import numpy as np

from ..engine import GlobalPositioningProblem, MapperScene, RotationAveragingProblem
from ..synthetic import qvec_to_rotmat
from . import base
from .keypoint_adjustment import default_context
from .mapping import IncrementalMapper, bundle_adjust, finish, gauge_component, triangulate_registered
from .reconstruction import Reconstruction
from .triangulation import TrackTriangulator, flatten_tracks

POSITIONAL_CONFIGS = ("CALIBRATED", "PLANAR")      # pairs that carry a baseline; a PANORAMIC pair carries a rotation only
ROTATION_CONFIGS = POSITIONAL_CONFIGS + ("PANORAMIC",)
RESIDUAL_BINS = (0.0, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 45.0, 90.0, 180.0)     # degrees: summary["residual_histogram"]


def view_graph(index_of_name, pairs, geometries):
    """The pairs a global mapper can use, on flat arrays: geometries with `success` whose `config` is absent, CALIBRATED or PLANAR
    (rotation and baseline) or PANORAMIC (rotation only: positional False), between two different known images, with a positive
    `num_inliers` (the pair's weight; 1 where the geometry carries none).  Returns
    dict(pair_image (P, 2) int32, pair_qvec (P, 4), pair_tvec (P, 3), num_inliers (P,), positional (P,) bool, index (P,) into
    `pairs`)."""
    rows = []
    for p, ((a, b), g) in enumerate(zip(pairs, geometries)):
        i, j = index_of_name.get(a), index_of_name.get(b)
        if not g.get("success") or i is None or j is None or i == j:
            continue
        config = g.get("config")
        if config is not None and config not in ROTATION_CONFIGS:
            continue
        q = np.asarray(g["qvec"], dtype=np.float64).reshape(4)
        t = np.asarray(g.get("tvec", np.zeros(3)), dtype=np.float64).reshape(3)
        if not (np.isfinite(q).all() and np.linalg.norm(q) > 0.0):
            continue
        weight = float(g.get("num_inliers", 1))
        if not (weight > 0.0 and np.isfinite(weight)):                  # a pair without weight joins nothing in the averaging
            continue
        positional = config in (None,) + POSITIONAL_CONFIGS and bool(np.isfinite(t).all()) and np.linalg.norm(t) > 0.0
        rows.append((i, j, q, t / np.linalg.norm(t) if positional else np.zeros(3), weight, positional, p))
    return dict(pair_image=np.array([(r[0], r[1]) for r in rows], np.int32).reshape(-1, 2),
                pair_qvec=np.array([r[2] for r in rows], np.float64).reshape(-1, 4),
                pair_tvec=np.array([r[3] for r in rows], np.float64).reshape(-1, 3),
                num_inliers=np.array([r[4] for r in rows], np.float64), positional=np.array([r[5] for r in rows], bool),
                index=np.array([r[6] for r in rows], np.int64))


def largest_component(n_images, pair_image, must_hold=None):
    """The mask (n_images,) of the largest connected component of the graph by image count (ties: the one that holds the lowest
    image index); with must_hold, the component of that image instead."""
    label = np.arange(n_images)

    def find(x):
        while label[x] != x:
            label[x] = label[label[x]]
            x = label[x]
        return x
    for i, j in np.asarray(pair_image, dtype=np.int64).reshape(-1, 2):
        a, b = find(i), find(j)
        if a != b:
            label[max(a, b)] = min(a, b)                       # the root of a component is its lowest image index
    roots = np.array([find(k) for k in range(n_images)], np.int64)
    if must_hold is not None:
        return roots == roots[must_hold]
    if n_images == 0:
        return np.zeros(0, bool)
    count = np.bincount(roots, minlength=n_images)
    return roots == int(np.argmax(count))                      # the first of equals = the lowest root


def positioning_graph(vg, use, angle, max_residual, root, n_images):
    """What goes on to the positioning once the rotations are averaged (host logic): `use` marks the rows of the view graph `vg`
    that were averaged and `angle` holds their residuals in degrees.  Pairs above max_residual leave; connectivity is recomputed
    from `root` over the others, and pairs and images that are cut off leave too.  Returns dict(above: rows of vg over the
    residual, rows: rows of vg that take part, comp: mask (n_images,) of the images that stay, weight: per row of `rows` the
    positioning weight -- num_inliers, 0 for a pair without a baseline)."""
    used = np.flatnonzero(use)
    above = np.asarray(angle) > float(max_residual)
    stay = used[~above]
    comp = largest_component(n_images, vg["pair_image"][stay], must_hold=root)
    rows = stay[comp[vg["pair_image"][stay, 0]]]
    return dict(above=used[above], rows=rows, comp=comp, weight=np.where(vg["positional"][rows], vg["num_inliers"][rows], 0.0))


def baseline_directions(qvec, pair_image, pair_tvec):
    """b_p = -R_j^t t_p / |t_p| per pair (unit; (1, 0, 0) where t_p is zero): the direction of c_j - c_i in the world."""
    out = np.tile([1.0, 0.0, 0.0], (len(pair_image), 1))
    for p, (_, j) in enumerate(np.asarray(pair_image).reshape(-1, 2)):
        t = pair_tvec[p]
        if np.linalg.norm(t) > 0.0:
            b = -qvec_to_rotmat(qvec[j]).T @ t
            out[p] = b / np.linalg.norm(b)
    return out


def rotation_averaging(names, pairs, geometries, conf=None, ctx=None):
    """Absolute rotations from relative ones: names (all images), pairs [(name1, name2)] and geometries as TwoViewVerifier /
    TwoViewClassifier return them.  Runs over the largest connected component of the usable pairs (view_graph); conf over
    GlobalMapper.default_conf['rotation_averaging'].  Returns ({name: qvec} of the component, root name, {pair: residual angle in
    degrees} of the pairs used)."""
    opts = base.merge_conf(GlobalMapper.default_conf['rotation_averaging'], conf)
    names = list(names)
    vg = view_graph({n: k for k, n in enumerate(names)}, list(pairs), list(geometries))
    comp = largest_component(len(names), vg["pair_image"])
    use = comp[vg["pair_image"][:, 0]] if len(vg["index"]) else np.zeros(0, bool)
    if comp.sum() < 2 or not use.any():
        return {}, None, {}
    local = np.cumsum(comp) - 1
    prob = RotationAveragingProblem(ctx or default_context(), int(comp.sum()), local[vg["pair_image"][use]], vg["pair_qvec"][use],
                                    vg["num_inliers"][use])
    d_q, root, _, d_angle = prob.solve(**opts)
    q, angle = d_q.download(), np.degrees(d_angle.download())
    members = np.flatnonzero(comp)
    return ({names[k]: q[x] for x, k in enumerate(members)}, names[members[root]],
            {tuple(pairs[p]): float(a) for p, a in zip(vg["index"][use], angle)})


class GlobalMapper:
    """Verified matches in, registered images and points out, without an initial pair: rotation averaging, global positioning,
    then the incremental mapper's triangulation, bundle adjustment and filter."""
    default_conf = {
        'max_rotation_residual': 10.0,       # degrees: pairs above it after the averaging do not take part in the positioning
        'min_num_observations': 15,          # an image that ends with fewer observations in tracks is taken out again
        'filter_max_reproj_error': 4.0,      # pixels
        'ba_max_num_iterations': 50,
        'ba_refine_focal_length': False,
        'rotation_averaging': {'l1_iterations': 20, 'max_iterations': 40, 'min_angle': 1e-3, 'sigma': 5.0, 'tolerance': 1e-10},
        'positioning': {'iterations': 8, 'cheirality_from': 2, 'sigma_obs': 1.0, 'sigma_pair': 3.0, 'min_det': 1e-12},
        'triangulation': {k: v for k, v in TrackTriangulator.default_conf.items() if k != 'refine'},
    }

    def __init__(self, conf=None, ctx=None):
        self.conf = base.merge_conf(self.default_conf, conf)
        c = self.conf
        if not 0.0 < float(c['max_rotation_residual']) <= 180.0:
            raise ValueError("max_rotation_residual must be in (0, 180] degrees")
        if int(c['min_num_observations']) < 0:
            raise ValueError("min_num_observations must not be negative")
        if int(c['ba_max_num_iterations']) < 1:
            raise ValueError("ba_max_num_iterations must be at least 1")
        if not float(c['filter_max_reproj_error']) > 0.0:
            raise ValueError("filter_max_reproj_error must be positive")
        if int(c['rotation_averaging']['max_iterations']) < 1 or int(c['positioning']['iterations']) < 1:
            raise ValueError("rotation_averaging.max_iterations and positioning.iterations must be at least 1")
        self.ctx = ctx

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: a dict over default_conf; unknown keys raise ValueError."""
        return cls(conf, ctx)

    @staticmethod
    def _gauge(st, registered, root):
        """What the bundle adjustment holds constant: the root's pose and the largest translation component of the registered image
        whose centre is farthest from the root's."""
        centre = np.array([-qvec_to_rotmat(q).T @ t for q, t in zip(st["qvec"], st["tvec"])])
        dist = np.where(registered, np.linalg.norm(centre - centre[root], axis=1), -1.0)
        far = int(np.argmax(dist))
        st["init"], st["gauge"] = (int(root), far), gauge_component(st["tvec"][far])

    def reconstruct(self, cameras, keypoints, graph, pairs, geometries, track_labels=None):
        """Arguments and return value as IncrementalMapper.reconstruct.  summary: status ("ok", "no_view_graph": fewer than two images
        joined by usable pairs, or no observations; "degenerate": the positioning met a singular system), root, num_reg_images,
        unregistered, rotation_iterations, residual_histogram (counts over RESIDUAL_BINS, degrees), pairs_above_max_residual,
        positioning_rounds, zero_weight_observations / zero_weight_pairs (shares after the positioning), positioning_pairs {pair: its
        final weight in the positioning}, panoramic_pairs, gauge_image, kernel_ms,
        final_ba, num_filtered_observations, mean_reprojection_error, num_points3D."""
        c = self.conf
        pairs, geometries = list(pairs), list(geometries)
        if len(pairs) != len(geometries):
            raise ValueError("pairs and geometries must have the same length")
        ctx = self.ctx or default_context()
        skeleton = IncrementalMapper._skeleton(cameras, keypoints)
        if track_labels is None:
            track_labels = base.compute_track_labels(graph)
        flat = flatten_tracks(skeleton, keypoints, graph, track_labels)
        names = [skeleton.images[i].name for i in flat["image_ids"]]
        index_of_name = {nm: k for k, nm in enumerate(names)}
        cam_size = np.array([[skeleton.cameras[k].width, skeleton.cameras[k].height] for k in flat["camera_ids"]], np.int32).reshape(-1, 2)
        n = len(names)
        st = dict(ctx=ctx, image_camera=flat["image_camera"], cam_model=flat["cam_model"], cam_params=flat["cam_params"].copy(),
                  qvec=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), tvec=np.zeros((n, 3)),
                  ms=dict(rotation_averaging=0.0, global_positioning=0.0, triangulate=0.0, bundle_adjustment_wall=0.0))
        summary = dict(status="no_view_graph", root=None, num_reg_images=0, unregistered=list(names), num_points3D=0, kernel_ms=st["ms"])
        vg = view_graph(index_of_name, pairs, geometries)
        comp = largest_component(n, vg["pair_image"])
        if n < 2 or len(vg["index"]) == 0 or comp.sum() < 2 or len(flat["obs_image"]) == 0:
            return Reconstruction(), summary
        st["scene"] = MapperScene(None, dict(flat, cam_size=cam_size))

        # -- rotation averaging over the component ------------------------------------------------------------------------------
        use = comp[vg["pair_image"][:, 0]]
        members = np.flatnonzero(comp)
        local = np.cumsum(comp) - 1
        ra = RotationAveragingProblem(ctx, len(members), local[vg["pair_image"][use]], vg["pair_qvec"][use], vg["num_inliers"][use])
        d_q, root_local, iterations, d_angle = ra.solve(timed=True, **c['rotation_averaging'])
        st["ms"]["rotation_averaging"] += sum(ra.kernel_ms.values())
        st["qvec"][members] = d_q.download()
        angle = np.degrees(d_angle.download())
        root = int(members[root_local])
        pg = positioning_graph(vg, use, angle, c['max_rotation_residual'], root, n)
        summary.update(root=names[root], rotation_iterations=iterations, residual_histogram=np.histogram(angle, RESIDUAL_BINS)[0].tolist(),
                       pairs_above_max_residual=[tuple(pairs[p]) for p in vg["index"][pg["above"]]],
                       panoramic_pairs=[tuple(pairs[p]) for p in vg["index"][use][~vg["positional"][use]]])

        # -- global positioning over what stays connected to the root without the pairs above the residual ----------------------
        comp, rows = pg["comp"], pg["rows"]
        members = np.flatnonzero(comp)
        if len(members) < 2:
            return Reconstruction(), summary
        local = np.cumsum(comp) - 1
        r = st["scene"].restricted_tracks(comp)
        b = baseline_directions(st["qvec"], vg["pair_image"][rows], vg["pair_tvec"][rows])
        gp = GlobalPositioningProblem(ctx, dict(track_offsets=r["track_offsets"], obs_image=local[r["obs_image"]], obs_xy=r["obs_xy"],
                                               image_camera=st["image_camera"][members], qvec=st["qvec"][members],
                                               cam_model=st["cam_model"], cam_params=st["cam_params"]),
                                      local[vg["pair_image"][rows]], b, pg["weight"], local[root])
        out = gp.solve(timed=True, **c['positioning'])
        st["ms"]["global_positioning"] += sum(gp.kernel_ms.values())
        w_obs, w_pair = out["obs_weight"].download()[:gp.n_obs], out["pair_weight"].download()[:gp.n_pairs]
        summary.update(positioning_rounds=out["rounds"], zero_weight_observations=float((w_obs == 0.0).mean()) if gp.n_obs else 0.0,
                       zero_weight_pairs=float((w_pair == 0.0).mean()) if gp.n_pairs else 0.0,
                       positioning_pairs={tuple(pairs[p]): float(w) for p, w in zip(vg["index"][rows], w_pair)},
                       positioning_kernel_ms=dict(gp.kernel_ms), rotation_kernel_ms=dict(ra.kernel_ms))
        if out["status"] != 0:
            summary["status"] = "degenerate"
            return Reconstruction(), summary
        centre = out["centre"].download()
        for x, k in enumerate(members):
            st["tvec"][k] = -qvec_to_rotmat(st["qvec"][k]) @ centre[x]
        summary["status"] = "ok"

        # -- refinement with the incremental mapper's stages ----------------------------------------------------------------------
        registered = comp.copy()
        t0 = time.perf_counter()
        self._gauge(st, registered, root)
        summary["gauge_image"] = names[st["init"][1]]
        tri = triangulate_registered(c, st, registered)
        if tri is None:                                                     # (a component without observations)
            summary["status"] = "no_view_graph"
            return Reconstruction(), summary
        bundle_adjust(c, st, registered, tri[1], tri[2])
        rec = finish(c, st, skeleton, flat, keypoints, registered, summary)
        kept = np.array([sum(p.point3D_id != -1 for p in rec.images[flat["image_ids"][k]].points2D) if registered[k] else 0 for k in range(n)])
        thin = registered & (kept < int(c['min_num_observations']))
        if thin.any() and (registered & ~thin).sum() >= 2:                 # take them out and finish again over the others
            registered &= ~thin
            self._gauge(st, registered, root if registered[root] else int(np.flatnonzero(registered)[0]))
            rec = finish(c, st, skeleton, flat, keypoints, registered, summary)
        summary["refinement_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        summary["unregistered"] = [names[k] for k in np.flatnonzero(~registered)]
        return rec, summary
