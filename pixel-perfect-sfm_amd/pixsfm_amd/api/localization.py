"""Mirror of pixsfm's query keypoint adjustment (QKA) for the accelerated path:
`QueryKeypointAdjuster(conf).refine(pnp_points2D, fmap, references, point2D_idxs)`
(pixsfm/localization/main.py:89-192) and the `_localization.QueryKeypointOptimizer` it drives
(pixsfm/localization/bindings.cc:36-57, src/single_query_keypoint_optimizer.h:86-222).

One Ceres problem over all 2D-3D correspondences of a query, one FeatureReference2DCostFunctor
block per (keypoint, reference descriptor), box bounds from the patch extent and `bound`
(src/query_keypoint_optimizer.h:141-172).  Here: one pxr_ka_solve sub-problem whose terms are the
unary reference terms of pxr_ka_view; the keypoints are independent 2x2 components of it.

`QueryBundleAdjuster(conf).refine(qvec, tvec, camera, points3D, fmap, references, inliers,
point2D_idxs)` (main.py:194-258; src/single_query_bundle_optimizer.h:91-222, query_bundle_optimizer.h:
114-151) is the one-image BA: FeatureReferenceCostFunctor blocks against CONSTANT 3D points, pose on
the quaternion manifold, intrinsics constant unless refine_* says otherwise.  It runs on pxr_ba_solve
with every (correspondence, reference descriptor) pair as its own constant point.

`absolute_pose_estimation(points2D, points3D, camera, estimation_options, refinement_options)` stands in for
pycolmap.absolute_pose_estimation (main.py:458), which is not installable here: a batched, deterministic P3P estimator with
local optimisation on the GPU (pxr_absolute_pose; DESIGN.md section 19 -- NOT COLMAP's LO-RANSAC).
`absolute_pose_estimation_batch` runs many queries in one launch.

`QueryLocalizer(reconstruction, conf, dense_features=..., references=...).localize(...)` is main.py:261-499 step by step:
query features, the references of the query (nearest / robust_mean / all_observations), QKA, PnP, unique inliers
(find_unique_inliers, find_unique_min_by_group, find_unique_min_reproj_inliers, compute_reprojection_errors: main.py:38-86),
QBA, the final inlier recount.  The 2D-3D pairs come from descriptor matching against the map's images
(api.matching: DescriptorMatcher + pairs_2d3d_from_matches); image retrieval, which picks those
images, stays outside (control plane).
"""
from collections import OrderedDict
from copy import deepcopy
from pathlib import Path

import numpy as np

from ..engine import AbsolutePoseProblem, BAProblem, lm_options, make_loss, nearest_references
from ..ka_engine import KAProblem
from . import base, features
from .keypoint_adjustment import default_context


def resolve_level_indices(level_indices, n_levels):      # pixsfm/util/misc.py:19-23
    if level_indices not in [None, "all"]:
        return level_indices
    return list(reversed(range(n_levels)))


def _reference_descriptors(ref):
    """The descriptors one correspondence contributes (single_query_keypoint_optimizer.h:86-222)."""
    if isinstance(ref, features.Reference):
        return ref.observations if ref.has_observations() else [ref.descriptor]
    if isinstance(ref, (list, tuple)):
        return [np.asarray(r, dtype=np.float64).reshape(1, -1) for r in ref]
    return [np.asarray(ref, dtype=np.float64).reshape(1, -1)]


def _build_problem(keypoints, fmap, references, patch_idxs, inliers, per_keypoint_problems=False):
    n = len(keypoints)
    if len(references) != n:
        raise ValueError("references.size() != keypoints.rows()")           # THROW_CHECK_EQ, :96 / :134 / :180
    if patch_idxs is not None and len(patch_idxs) != n:
        raise ValueError("patch_idxs.size() != keypoints.rows()")           # :70-72
    rows, patches, unary_node, unary_ref = [], [], [], []
    for idx in range(n):
        if inliers is not None and not inliers[idx]:
            continue
        descs = _reference_descriptors(references[idx])
        if not descs:
            continue                                                        # added_to_problem == false, :140-154
        node = len(rows)
        rows.append(idx)
        patches.append(fmap.fpatch(idx if patch_idxs is None else patch_idxs[idx]))
        for d in descs:
            unary_node.append(node)
            unary_ref.append(d.reshape(-1))
    m = len(rows)
    prob = dict(kp=np.asarray(keypoints, dtype=np.float64)[rows].reshape(-1, 2),
                node_patch=np.arange(m, dtype=np.int64), node_const=np.zeros(m, np.uint8),
                node_problem=np.arange(m, dtype=np.int32) if per_keypoint_problems else np.zeros(m, np.int32),
                edge_src=np.zeros(0, np.int32), edge_dst=np.zeros(0, np.int32), edge_w=np.zeros(0),
                unary_node=np.asarray(unary_node, dtype=np.int32),
                unary_ref=(np.asarray(unary_ref, dtype=np.float64).reshape(len(unary_node), -1) if unary_node else np.zeros((0, 0))),
                unary_w=None)      # no residual at all (every correspondence an outlier): the callers return False
    return rows, patches, prob


def find_feature_inliers(p2Ds, fmap, references, interpolation_config, thresh=-1, ctx=None):
    """localization/main.py:20-35: keep a correspondence when |f(patch_i, p2D_i) - reference_i| <= thresh
    (only array references are tested; patch index = correspondence index, as in the reference).
    The descriptor distances come from the device: one zero-iteration sub-problem per keypoint,
    whose initial cost is 0.5 |f - ref|^2 under the trivial loss."""
    inliers = [True] * len(p2Ds)
    if thresh < 0.0 or len(p2Ds) == 0:
        return inliers
    tested = [i for i, r in enumerate(references) if isinstance(r, np.ndarray)]
    if not tested:
        return inliers
    ic = interpolation_config if isinstance(interpolation_config, base.InterpolationConfig) \
        else base.InterpolationConfig(interpolation_config)
    ctx = ctx or default_context()
    mask = [i in set(tested) for i in range(len(p2Ds))]
    rows, patches, prob = _build_problem(np.asarray(p2Ds, dtype=np.float64), fmap, references, None, mask,
                                         per_keypoint_problems=True)
    arena = features.to_arena(ctx, patches)
    prob['node_patch'] = arena.index
    ka = KAProblem(ctx, arena, prob)
    _, per = ka.solve(ic.to_engine(), make_loss('trivial', []), bound=0.0, options=lm_options(max_iterations=0),
                      per_problem=True)
    arena.close()
    for i, s in zip(rows, per):
        if np.sqrt(2.0 * s['initial_cost']) > thresh:
            inliers[i] = False
    return inliers


def find_nearest_references(query_fmap, references, keypoints, point3D_ids, interpolation_config, patch_idxs=None,
                            ctx=None):
    """_localization.find_nearest_references (bindings.cc:60; src/nearest_references.h:20-52): for every
    2D-3D correspondence, the observation descriptor of its 3D point's Reference that is nearest to the
    query descriptor interpolated at the keypoint.  `references`: {point3D_id: Reference} extracted with
    keep_observations=True.  Returns a list of (1, C) arrays."""
    ic = interpolation_config if isinstance(interpolation_config, base.InterpolationConfig) \
        else base.InterpolationConfig(interpolation_config)
    keypoints = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2)
    n = len(keypoints)
    if len(point3D_ids) != n or (patch_idxs is not None and len(patch_idxs) != n):
        raise ValueError("keypoints, point3D_ids and patch_idxs must have the same length")
    if n == 0:
        return []
    cand, ptr = [], [0]
    for pid in point3D_ids:
        ref = references[pid]
        if not ref.has_observations():
            raise ValueError("Missing observations in references. Extract references with option "
                             "keep_observations=True.")                     # THROW_CHECK_MSG, :33-35
        cand.extend(o.reshape(-1) for o in ref.observations)
        ptr.append(len(cand))
    ctx = ctx or default_context()
    patches = [query_fmap.fpatch(i if patch_idxs is None else patch_idxs[i]) for i in range(n)]
    arena = features.to_arena(ctx, patches)
    cand = np.asarray(cand, dtype=np.float64)
    best, _, _ = nearest_references(ctx, arena, ic.to_engine(), keypoints, arena.index, ptr, cand)
    arena.close()
    return [cand[b].reshape(1, -1).copy() for b in best]


class QueryKeypointOptimizer:
    """_localization.QueryKeypointOptimizer: ctor (options, interpolation_config);
    run(keypoints, fmap, references, patch_idxs=None, inliers=None) refines `keypoints` in place and
    returns False when the problem has no residuals (query_keypoint_optimizer.h:56-59)."""

    # the C++ struct's own defaults (query_refinement_options.h:60-95); QueryKeypointAdjuster.default_conf carries the
    # Python-level ones (bound 4, parameter_tolerance 1e-5) and always passes them in full
    option_defaults = {
        'loss': {'name': 'trivial', 'params': []},
        'solver': {**base.solver_default_conf, 'parameter_tolerance': 1e-04, 'callbacks': []},
        'print_summary': True, 'bound': -1.0,
    }

    def __init__(self, options=None, interpolation_config=None, ctx=None):
        self.options = base.merge_conf(self.option_defaults, options)
        ic = interpolation_config
        self.interpolation = ic if isinstance(ic, base.InterpolationConfig) else base.InterpolationConfig(ic)
        self.ctx = ctx
        self.last_summary = None

    def run(self, keypoints, fmap, references, patch_idxs=None, inliers=None):
        keypoints = np.asarray(keypoints)
        if keypoints.ndim != 2 or keypoints.shape[1] != 2 or keypoints.dtype != np.float64:
            raise ValueError("keypoints must be an (N, 2) float64 array (refined in place)")
        rows, patches, prob = _build_problem(keypoints, fmap, references, patch_idxs, inliers)
        if len(prob['unary_node']) == 0:
            return False
        ctx = self.ctx or default_context()
        arena = features.to_arena(ctx, patches)
        prob['node_patch'] = arena.index
        o, s = self.options, self.options['solver']
        # ParameterizeKeypoint: bounds when bound > 0 or the map is sparse (:145); the accelerated
        # path holds sparse maps only (features.to_arena), so the patch box always applies.
        ka = KAProblem(ctx, arena, prob)
        lm = lm_options(max_iterations=s['max_num_iterations'], function_tolerance=s['function_tolerance'],
                        gradient_tolerance=s['gradient_tolerance'], parameter_tolerance=s['parameter_tolerance'],
                        max_consecutive_invalid_steps=s['max_num_consecutive_invalid_steps'])
        total, _ = ka.solve(self.interpolation.to_engine(), make_loss(o['loss']['name'], o['loss']['params']),
                            bound=o['bound'], options=lm)
        keypoints[rows] = ka.keypoints()
        self.last_summary = total
        arena.close()
        return True

    def run_batch(self, queries):
        """Many queries in ONE launch ("batch across queries for throughput"): `queries` is a list of
        (keypoints, fmap, references, patch_idxs | None, inliers | None) tuples with run()'s meaning.  Each query
        is its own sub-problem -- its own trust region, step acceptance and termination, exactly as if run() had
        been called on it -- but all of them share one arena upload and one pxr_ka_solve call.  Returns the list
        of run()'s booleans; per-query summaries in self.last_summaries."""
        built = []
        for q in queries:
            keypoints, fmap, references = q[0], q[1], q[2]
            patch_idxs = q[3] if len(q) > 3 else None
            inliers = q[4] if len(q) > 4 else None
            keypoints = np.asarray(keypoints)
            if keypoints.ndim != 2 or keypoints.shape[1] != 2 or keypoints.dtype != np.float64:
                raise ValueError("keypoints must be an (N, 2) float64 array (refined in place)")
            built.append((keypoints,) + _build_problem(keypoints, fmap, references, patch_idxs, inliers))
        live = [i for i, b in enumerate(built) if len(b[3]['unary_node'])]
        ok = [False] * len(queries)
        self.last_summaries = [None] * len(queries)
        if not live:
            return ok
        patches, parts, n0, u0 = [], [], 0, 0
        for slot, i in enumerate(live):
            _, rows, plist, prob = built[i]
            m = len(rows)
            patches += plist
            parts.append(dict(kp=prob['kp'], node_patch=prob['node_patch'] + n0, node_problem=np.full(m, slot, np.int32),
                              unary_node=prob['unary_node'] + n0, unary_ref=prob['unary_ref']))
            n0 += m
        cat = {k: np.concatenate([p_[k] for p_ in parts]) for k in parts[0]}
        cat.update(node_const=np.zeros(n0, np.uint8), edge_src=np.zeros(0, np.int32), edge_dst=np.zeros(0, np.int32),
                   edge_w=np.zeros(0), unary_w=None)
        ctx = self.ctx or default_context()
        arena = features.to_arena(ctx, patches)
        cat['node_patch'] = arena.index[cat['node_patch']]
        o, s = self.options, self.options['solver']
        ka = KAProblem(ctx, arena, cat)
        lm = lm_options(max_iterations=s['max_num_iterations'], function_tolerance=s['function_tolerance'],
                        gradient_tolerance=s['gradient_tolerance'], parameter_tolerance=s['parameter_tolerance'],
                        max_consecutive_invalid_steps=s['max_num_consecutive_invalid_steps'])
        total, per = ka.solve(self.interpolation.to_engine(), make_loss(o['loss']['name'], o['loss']['params']),
                              bound=o['bound'], options=lm, per_problem=True)
        out = ka.keypoints()
        n0 = 0
        for slot, i in enumerate(live):
            keypoints, rows = built[i][0], built[i][1]
            keypoints[rows] = out[n0:n0 + len(rows)]
            n0 += len(rows)
            ok[i] = True
            self.last_summaries[i] = per[slot]
        self.last_summary = total
        arena.close()
        return ok


class QueryKeypointAdjuster:
    """pixsfm/localization/main.py:89-192."""

    default_conf = {
        'apply': True,
        'feature_inlier_thresh': -1,
        'interpolation': base.interpolation_default_conf,
        'level_indices': None,
        'stack_correspondences': False,
        'optimizer': {
            'loss': {'name': 'trivial', 'params': []},
            'solver': {**base.solver_default_conf, 'parameter_tolerance': 1e-05},
            'print_summary': False,
            'bound': 4.0,
        },
    }

    def __init__(self, conf=None, callbacks=None, ctx=None):
        self.conf = base.merge_conf(deepcopy(self.default_conf), conf)
        self.ctx = ctx
        self.solver = QueryKeypointOptimizer(self.conf['optimizer'], self.conf['interpolation'], ctx=ctx)

    def refine(self, pnp_points2D, fmap, references, point2D_idxs=None):
        qka_inliers = find_feature_inliers(pnp_points2D, fmap, references, self.conf['interpolation'],
                                           thresh=self.conf['feature_inlier_thresh'], ctx=self.ctx)
        if self.conf['stack_correspondences']:
            self.refine_stacked(pnp_points2D, fmap, references, point2D_idxs, inliers=qka_inliers)
        else:
            self.solver.run(pnp_points2D, fmap, references, patch_idxs=point2D_idxs, inliers=qka_inliers)

    def refine_multilevel(self, pnp_points2D, query_fmaps, references, point2D_idxs=None):
        for l_idx in resolve_level_indices(self.conf['level_indices'], len(query_fmaps)):
            self.refine(pnp_points2D, query_fmaps[l_idx], references[l_idx], point2D_idxs=point2D_idxs)

    def refine_batch(self, queries):
        """refine() for many queries at once: `queries` = [(pnp_points2D, fmap, references, point2D_idxs | None), ...];
        one GPU launch, each query solved as its own problem (not available with stack_correspondences)."""
        if self.conf['stack_correspondences']:
            raise ValueError("refine_batch does not stack correspondences; call refine() per query")
        batch = []
        for q in queries:
            pts, fmap, refs = q[0], q[1], q[2]
            idxs = q[3] if len(q) > 3 else None
            inl = find_feature_inliers(pts, fmap, refs, self.conf['interpolation'],
                                       thresh=self.conf['feature_inlier_thresh'], ctx=self.ctx)
            batch.append((pts, fmap, refs, idxs, inl))
        return self.solver.run_batch(batch)

    def refine_stacked(self, pnp_points2D, fmap, references, point2D_idxs, inliers=None):
        if point2D_idxs is None:
            raise ValueError("point2D_idxs must not be None in stacked QKA.")
        unique_p2D_idxs = list(dict.fromkeys(point2D_idxs))
        pos = {p: i for i, p in enumerate(unique_p2D_idxs)}
        old_to_new = [pos[p] for p in point2D_idxs]
        unique_kps = np.zeros((len(unique_p2D_idxs), 2), dtype=np.float64)
        for idx, new in enumerate(old_to_new):
            unique_kps[new] = pnp_points2D[idx]
        stacked_refs = [[] for _ in unique_p2D_idxs]
        for idx, query_ref in enumerate(references):
            if not isinstance(query_ref, np.ndarray):
                raise ValueError("Stacked QKA requires a np.ndarray reference for each 2D-3D correspondence. "
                                 "Consider setting target_references='nearest'.")
            stacked_refs[old_to_new[idx]].append(query_ref)
        # the reference forwards the per-correspondence inlier list to the per-keypoint problem
        # (main.py:186-188); it only has the right length when every point2D_idx is unique
        run_inliers = inliers if inliers is not None and len(inliers) == len(unique_p2D_idxs) else None
        self.solver.run(unique_kps, fmap, stacked_refs, patch_idxs=unique_p2D_idxs, inliers=run_inliers)
        for i in range(len(point2D_idxs)):
            pnp_points2D[i] = unique_kps[old_to_new[i]]


def _qba_observations(points3D, fmap, references, inliers, patch_idxs):
    """The residual blocks of a query BA (single_query_bundle_optimizer.h:92-221): one per correspondence and reference
    descriptor, inlier correspondences only, in that order.  -> (correspondence index, patch, xyz, descriptor) lists."""
    rows, patches, xyz, refs = [], [], [], []
    for idx in range(len(points3D)):
        if inliers is not None and not inliers[idx]:
            continue
        patch = fmap.fpatch(idx if patch_idxs is None else patch_idxs[idx])
        for d in _reference_descriptors(references[idx]):
            rows.append(idx)
            patches.append(patch)
            xyz.append(np.asarray(points3D[idx], dtype=np.float64).reshape(3))
            refs.append(d.reshape(-1))
    return rows, patches, xyz, refs


def _qba_camera_mask(camera, options):
    """ParameterizeQuery (query_bundle_optimizer.h:113-146): bit mask of the camera parameters held constant."""
    K = len(camera.params)
    if not (options['refine_focal_length'] or options['refine_principal_point'] or options['refine_extra_params']):
        return (1 << K) - 1                                                   # :121-126
    const = []
    if not options['refine_focal_length']:
        const += camera.focal_length_idxs()
    if not options['refine_principal_point']:
        const += camera.principal_point_idxs()
    if not options['refine_extra_params']:
        const += camera.extra_params_idxs()
    return sum(1 << a for a in const)


class QueryBundleOptimizer:
    """_localization.QueryBundleOptimizer: ctor (options, interpolation_config);
    run(qvec, tvec, camera, points3D, fmap, references, inliers=None, patch_idxs=None) refines qvec,
    tvec (numpy arrays) and camera.params in place; False when no residual was added."""

    # the C++ struct's own defaults (query_refinement_options.h:8-57)
    option_defaults = {
        'loss': {'name': 'cauchy', 'params': [0.25]},
        'solver': {**base.solver_default_conf, 'parameter_tolerance': 1e-05, 'callbacks': []},
        'print_summary': True,
        'refine_focal_length': False, 'refine_principal_point': False, 'refine_extra_params': False,
    }

    def __init__(self, options=None, interpolation_config=None, ctx=None):
        self.options = base.merge_conf(self.option_defaults, options)
        ic = interpolation_config
        self.interpolation = ic if isinstance(ic, base.InterpolationConfig) else base.InterpolationConfig(ic)
        self.ctx = ctx
        self.last_summary = None
        self.last_summaries = None
        self.last_batch_path = None

    @staticmethod
    def _check(qvec, tvec, points3D, references, inliers, patch_idxs):
        n = len(points3D)
        if len(references) != n:
            raise ValueError("references.size() != points3D.size()")          # THROW_CHECK_EQ, :100 / :141 / :183
        if patch_idxs is not None and len(patch_idxs) != n:
            raise ValueError("patch_idxs.size() != points3D.size()")
        if inliers is not None and len(inliers) != n:
            raise ValueError("inliers.size() != points3D.size()")
        for name, v, k in (("qvec", qvec, 4), ("tvec", tvec, 3)):
            if not isinstance(v, np.ndarray) or v.dtype != np.float64 or v.size != k:
                raise ValueError("%s must be a float64 numpy array of %d values (refined in place)" % (name, k))

    def _problem(self, qvec, tvec, camera, points3D, fmap, references, inliers, patch_idxs):
        """The QBA problem at (qvec, tvec, camera): (BAProblem, arena, camera mask, number of residual blocks), or None when no
        residual is added -- one image, every point constant."""
        self._check(qvec, tvec, points3D, references, inliers, patch_idxs)
        rows, patches, xyz, refs = _qba_observations(points3D, fmap, references, inliers, patch_idxs)
        if not patches:
            return None
        ctx = self.ctx or default_context()
        arena = features.to_arena(ctx, patches)
        m = len(patches)
        q = qvec.reshape(4)
        params = np.zeros((1, 12))
        params[0, :len(camera.params)] = camera.params
        prob = dict(obs_image=np.zeros(m, np.int32), obs_point=np.arange(m, dtype=np.int32),
                    obs_patch=arena.index, image_camera=np.zeros(1, np.int32),
                    qvec=q.reshape(1, 4).copy(), tvec=tvec.reshape(1, 3).copy(),
                    cam_model=np.array([camera.model_id], np.int32), cam_params=params,
                    xyz=np.array(xyz), refs=np.array(refs))
        return BAProblem(ctx, arena, prob), arena, _qba_camera_mask(camera, self.options), m

    def run(self, qvec, tvec, camera, points3D, fmap, references, inliers=None, patch_idxs=None):
        built = self._problem(qvec, tvec, camera, points3D, fmap, references, inliers, patch_idxs)
        if built is None:
            return False
        ba, arena, cam_mask, m = built
        ctx = ba.ctx
        o, s = self.options, self.options['solver']
        K = len(camera.params)
        lm = lm_options(max_iterations=s['max_num_iterations'], function_tolerance=s['function_tolerance'],
                        gradient_tolerance=s['gradient_tolerance'], parameter_tolerance=s['parameter_tolerance'],
                        max_consecutive_invalid_steps=s['max_num_consecutive_invalid_steps'],
                        use_inner_iterations=False)     # every point is constant: nothing for inner iterations
        callbacks = list(s.get('callbacks') or [])
        if callbacks:
            ctx.set_iteration_callbacks(callbacks)
        try:
            summary = ba.solve(self.interpolation.to_engine(), make_loss(o['loss']['name'], o['loss']['params']),
                               np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.array([cam_mask], np.uint16),
                               np.ones(m, np.uint8), options=lm)
        finally:
            if callbacks:
                ctx.set_iteration_callbacks(None)
        q_out, t_out, cam_out, _ = ba.params()
        qvec.reshape(4)[:] = q_out[0]
        tvec.reshape(3)[:] = t_out[0]
        camera.params[:] = cam_out[0, :K]
        self.last_summary = summary
        arena.close()
        return True

    def batch_fallback_reason(self):
        """Why run_batch would call run() per query whatever the patches are, or None: the batch kernel keeps the intrinsics
        constant and calls nothing back (pxr_query_ba_solve)."""
        o = self.options
        if o['refine_focal_length'] or o['refine_principal_point'] or o['refine_extra_params']:
            return "the batch kernel keeps the intrinsics constant (refine_focal_length / refine_principal_point / refine_extra_params)"
        if list(o['solver'].get('callbacks') or []):
            return "the batch kernel runs its loop on the device and calls no iteration callbacks"
        return None

    def run_batch(self, queries):
        """Many queries in ONE launch (pxr_query_ba_solve: a workgroup per query, the trust-region loop inside the kernel):
        `queries` is a list of (qvec, tvec, camera, points3D, fmap, references, inliers | None, patch_idxs | None) tuples with
        run()'s meaning and checks.  Every qvec / tvec is refined in place; returns the list of run()'s booleans, the per-query
        summaries in self.last_summaries (None for a query without residuals).  All queries share one arena upload.
        With a refine_* option, with iteration callbacks, or with patches the batch kernel does not take (anything but fp16 /
        fp32 / fp64 patches of 128 or 64 channels and one shape) it calls run() per query -- unchanged results;
        self.last_batch_path says which path ran ("batch" or "per_query") and self.last_batch_reason why."""
        from ..engine import QueryBAProblem, query_ba_supported
        qs = []
        for q in queries:
            q = tuple(q)
            if not 6 <= len(q) <= 8:
                raise ValueError("a query is (qvec, tvec, camera, points3D, fmap, references[, inliers[, patch_idxs]])")
            q = q + (None,) * (8 - len(q))
            self._check(q[0], q[1], q[3], q[5], q[6], q[7])
            qs.append(q)
        reason = self.batch_fallback_reason()
        blocks, arena = [], None
        if reason is None:
            blocks = [_qba_observations(q[3], q[4], q[5], q[6], q[7]) for q in qs]
            patches = [p for b in blocks for p in b[1]]
            if patches:
                ctx = self.ctx or default_context()
                try:
                    arena = features.to_arena(ctx, patches)
                except ValueError as e:                     # patches of several shapes: no one arena
                    reason = str(e)
                if arena is not None and not query_ba_supported(arena):
                    reason = "no batch kernel for %s patches of %d channels" % (np.dtype(arena.dtype).name, int(arena.C))
                    arena.close()
        self.last_batch_reason = reason
        if reason is not None:
            self.last_batch_path = "per_query"
            ok, summaries = [], []
            for q in qs:
                ok.append(self.run(q[0], q[1], q[2], q[3], q[4], q[5], inliers=q[6], patch_idxs=q[7]))
                summaries.append(self.last_summary if ok[-1] else None)
            self.last_summaries = summaries
            return ok
        self.last_batch_path = "batch"
        ok = [len(b[1]) > 0 for b in blocks]
        self.last_summaries = [None] * len(qs)
        live = [i for i, has in enumerate(ok) if has]
        if not live:
            return ok
        o, s = self.options, self.options['solver']
        off = np.concatenate([[0], np.cumsum([len(blocks[i][1]) for i in live])]).astype(np.int64)
        params = np.zeros((len(live), 12))
        for slot, i in enumerate(live):
            params[slot, :len(qs[i][2].params)] = qs[i][2].params
        prob = dict(query_offsets=off, obs_patch=arena.index,
                    xyz=np.array([x for i in live for x in blocks[i][2]]), refs=np.array([r for i in live for r in blocks[i][3]]),
                    qvec=np.array([qs[i][0].reshape(4) for i in live]), tvec=np.array([qs[i][1].reshape(3) for i in live]),
                    query_camera=np.arange(len(live), dtype=np.int32),
                    cam_model=np.array([qs[i][2].model_id for i in live], np.int32), cam_params=params)
        lm = lm_options(max_iterations=s['max_num_iterations'], function_tolerance=s['function_tolerance'],
                        gradient_tolerance=s['gradient_tolerance'], parameter_tolerance=s['parameter_tolerance'],
                        max_consecutive_invalid_steps=s['max_num_consecutive_invalid_steps'], use_inner_iterations=False)
        try:
            qba = QueryBAProblem(ctx, arena, prob)
            per = qba.solve(self.interpolation.to_engine(), make_loss(o['loss']['name'], o['loss']['params']), options=lm)
            q_out, t_out = qba.poses()
        finally:
            arena.close()
        for slot, i in enumerate(live):
            qs[i][0].reshape(4)[:] = q_out[slot]
            qs[i][1].reshape(3)[:] = t_out[slot]
            self.last_summaries[i] = per[slot]
        return ok

    def covariance(self, qvec, tvec, camera, points3D, fmap, references, inliers=None, patch_idxs=None):
        """The 6 x 6 covariance of the query pose at (qvec, tvec) -- rotation in radians about the camera axes, then the
        translation -- from the problem run() solves (every point constant: the inverse of the pose block of J~^T J~, with the
        refined intrinsics marginalised when the options refine any); None when no residual is added.  Raises ValueError when the
        correspondences do not determine the pose."""
        from .covariance import half_angle_to_radians
        built = self._problem(qvec, tvec, camera, points3D, fmap, references, inliers, patch_idxs)
        if built is None:
            return None
        ba, arena, cam_mask, m = built
        o = self.options
        try:
            ba.eval(self.interpolation.to_engine(), with_jacobian=True)
            cov = ba.covariance(make_loss(o['loss']['name'], o['loss']['params']), np.zeros(1, np.uint8), np.zeros(1, np.uint8),
                                np.array([cam_mask], np.uint16), np.ones(m, np.uint8))
        finally:
            arena.close()
        if cov["summary"]["info"] != 0:
            raise ValueError("the query pose is not determined by its %d correspondences (rank deficient at column %d)"
                             % (m, cov["summary"]["info"]))
        return half_angle_to_radians(cov["pose"][0])


class QueryBundleAdjuster:
    """pixsfm/localization/main.py:194-258."""

    default_conf = {
        'apply': True,
        'interpolation': base.interpolation_default_conf,
        'level_indices': None,
        'optimizer': {
            'loss': {'name': 'cauchy', 'params': [0.25]},
            'solver': {**base.solver_default_conf},
            'print_summary': False,
            'refine_focal_length': False, 'refine_principal_point': False, 'refine_extra_params': False,
        },
    }

    def __init__(self, conf=None, callbacks=None, ctx=None):
        self.conf = base.merge_conf(deepcopy(self.default_conf), conf)
        self.solver = QueryBundleOptimizer(self.conf['optimizer'], self.conf['interpolation'], ctx=ctx)

    def refine(self, qvec, tvec, camera, points3D, fmap, references, inliers=None, point2D_idxs=None):
        return self.solver.run(qvec, tvec, camera, points3D, fmap, references, inliers=inliers,
                               patch_idxs=point2D_idxs)

    def refine_multilevel(self, qvec, tvec, camera, points3D, fmaps, references, inliers=None, point2D_idxs=None):
        assert len(fmaps) == len(references)
        for level in resolve_level_indices(self.conf['level_indices'], len(fmaps)):
            self.refine(qvec, tvec, camera, points3D, fmaps[level], references[level], inliers=inliers,
                        point2D_idxs=point2D_idxs)

    def refine_batch(self, queries):
        """refine() for many queries in one launch: `queries` = [(qvec, tvec, camera, points3D, fmap, references, inliers | None,
        point2D_idxs | None), ...]; every qvec / tvec is refined in place.  Returns refine()'s booleans
        (QueryBundleOptimizer.run_batch, which also says when it runs the queries one by one instead)."""
        return self.solver.run_batch(queries)

    def refine_multilevel_batch(self, queries):
        """refine_multilevel() for many queries: as refine_batch, with the `fmaps` and `references` of every level in place of
        fmap and references -- one launch per level over all queries.  Returns the booleans of the last level."""
        queries = [tuple(q) + (None,) * (8 - len(q)) for q in queries]
        if not queries:
            return []
        n_levels = len(queries[0][4])
        for q in queries:
            if len(q) != 8:
                raise ValueError("a query is (qvec, tvec, camera, points3D, fmaps, references[, inliers[, point2D_idxs]])")
            if len(q[4]) != len(q[5]) or len(q[4]) != n_levels:
                raise ValueError("every query needs fmaps and references of the same %d levels" % n_levels)
        ok = [False] * len(queries)
        for level in resolve_level_indices(self.conf['level_indices'], n_levels):
            ok = self.refine_batch([(q[0], q[1], q[2], q[3], q[4][level], q[5][level], q[6], q[7]) for q in queries])
        return ok

    def covariance(self, qvec, tvec, camera, points3D, fmaps, references, inliers=None, point2D_idxs=None):
        """QueryBundleOptimizer.covariance on the LAST level refine_multilevel refines (the finest by default)."""
        assert len(fmaps) == len(references)
        level = list(resolve_level_indices(self.conf['level_indices'], len(fmaps)))[-1]
        return self.solver.covariance(qvec, tvec, camera, points3D, fmaps[level], references[level], inliers=inliers,
                                      patch_idxs=point2D_idxs)


# ---- PnP ---------------------------------------------------------------------------------------------------------------------------
# pycolmap 0.x: AbsolutePoseEstimationOptions {estimate_focal_length, num_focal_length_samples, min_focal_length_ratio,
# max_focal_length_ratio, ransac: RANSACOptions}, AbsolutePoseRefinementOptions {gradient_tolerance, max_num_iterations,
# loss_function_scale, refine_focal_length, refine_extra_params, print_summary}
_RANSAC_KEYS = {"max_error": "max_error", "min_inlier_ratio": "min_inlier_ratio", "confidence": "confidence",
                "min_num_trials": "min_num_trials", "max_num_trials": "max_num_trials",
                # the estimator's own
                "min_num_inliers": "min_num_inliers", "round_size": "round_size", "seed": "seed", "lo_rounds": "lo_rounds"}
_REFINEMENT_KEYS = {"max_num_iterations": "refine_max_iterations", "loss_function_scale": "refine_loss_scale"}


def abspose_engine_options(estimation_options=None, refinement_options=None):
    """The keyword arguments of engine.abspose_options for the option dicts QueryLocalizer passes to
    pycolmap.absolute_pose_estimation.  Unknown keys raise ValueError; refining intrinsics raises NotImplementedError."""
    out = {}
    est = dict(estimation_options or {})
    if est.pop("estimate_focal_length", False):
        raise NotImplementedError("estimate_focal_length: the estimator takes the camera as given; refine intrinsics in the "
                                  "query bundle adjustment (QBA.optimizer.refine_focal_length)")
    ransac = est.pop("ransac", None) or {}
    if est:
        raise ValueError("unknown estimation option(s) %s" % sorted(est))
    for k, v in dict(ransac).items():
        if k not in _RANSAC_KEYS:
            raise ValueError("unknown RANSAC option %r" % (k,))
        out[_RANSAC_KEYS[k]] = v
    ref = dict(refinement_options or {})
    for k in ("refine_focal_length", "refine_extra_params"):
        if ref.pop(k, False):
            raise NotImplementedError("%s: the pose refinement keeps the intrinsics constant; refine them in the query bundle "
                                      "adjustment (QBA.optimizer.%s)" % (k, k))
    ref.pop("print_summary", None)
    ref.pop("gradient_tolerance", None)       # the refinement stops on its step norm
    for k, v in ref.items():
        if k not in _REFINEMENT_KEYS:
            raise ValueError("unknown refinement option %r" % (k,))
        out[_REFINEMENT_KEYS[k]] = v
    return out


def absolute_pose_estimation_batch(queries, estimation_options=None, refinement_options=None, ctx=None):
    """Many queries in ONE launch: `queries` = [(points2D (n, 2), points3D (n, 3), camera), ...].  Returns one dict per query
    as absolute_pose_estimation does."""
    opts = abspose_engine_options(estimation_options, refinement_options)
    queries = list(queries)
    if not queries:
        return []
    xy = [np.asarray(q[0], dtype=np.float64).reshape(-1, 2) for q in queries]
    xyz = [np.asarray(q[1], dtype=np.float64).reshape(-1, 3) for q in queries]
    for a, b in zip(xy, xyz):
        if len(a) != len(b):
            raise ValueError("points2D and points3D must have the same length")
    cams = [q[2] for q in queries]
    params = np.zeros((len(cams), 12))
    for i, c in enumerate(cams):
        params[i, :len(c.params)] = c.params
    off = np.concatenate([[0], np.cumsum([len(a) for a in xy])]).astype(np.int64)
    prob = dict(query_offsets=off, xy=np.concatenate(xy), xyz=np.concatenate(xyz), query_camera=np.arange(len(cams), dtype=np.int32),
                cam_model=np.array([c.model_id for c in cams], np.int32), cam_params=params)
    ctx = ctx or default_context()
    d_q, d_t, d_status, d_ninl, _, d_inl, _ = AbsolutePoseProblem(ctx, prob).estimate(**opts)
    q, t, status, ninl, inl = d_q.download(), d_t.download(), d_status.download(), d_ninl.download(), d_inl.download()
    out = []
    for i in range(len(queries)):
        if status[i] != 0:
            out.append({"success": False})
        else:
            out.append({"success": True, "qvec": q[i].copy(), "tvec": t[i].copy(), "num_inliers": int(ninl[i]),
                        "inliers": [bool(x) for x in inl[off[i]:off[i + 1]]]})
    return out


def absolute_pose_estimation(points2D, points3D, camera, estimation_options=None, refinement_options=None, ctx=None):
    """pycolmap.absolute_pose_estimation's shape: {"success", "qvec", "tvec", "num_inliers", "inliers"}, or {"success": False}."""
    return absolute_pose_estimation_batch([(points2D, points3D, camera)], estimation_options, refinement_options, ctx=ctx)[0]


# ---- unique inliers (main.py:38-86) --------------------------------------------------------------------------------------------------
def _world_to_image(model_id, k, u, v):
    r2 = u * u + v * v
    if model_id == 0:
        return np.stack([k[0] * u + k[1], k[0] * v + k[2]], 1)
    if model_id == 1:
        return np.stack([k[0] * u + k[2], k[1] * v + k[3]], 1)
    if model_id in (2, 3):
        rad = k[3] * r2 + (k[4] * r2 * r2 if model_id == 3 else 0.0)
        return np.stack([k[0] * u * (1 + rad) + k[1], k[0] * v * (1 + rad) + k[2]], 1)
    if model_id == 4:
        rad = k[4] * r2 + k[5] * r2 * r2
        du = u * rad + 2 * k[6] * u * v + k[7] * (r2 + 2 * u * u)
        dv = v * rad + 2 * k[7] * u * v + k[6] * (r2 + 2 * v * v)
        return np.stack([k[0] * (u + du) + k[2], k[1] * (v + dv) + k[3]], 1)
    raise NotImplementedError("compute_reprojection_errors: camera model %d without a camera.world_to_image" % model_id)


def compute_reprojection_errors(pnp_points2D, pnp_points3D, qvec, tvec, camera):
    """main.py:80-86: |camera.world_to_image(R X + t) - p2D| per correspondence, as a list."""
    X = np.asarray([getattr(p, "xyz", p) for p in pnp_points3D], dtype=np.float64).reshape(-1, 3)
    p2D = np.asarray(pnp_points2D, dtype=np.float64).reshape(-1, 2)
    q = np.asarray(qvec, dtype=np.float64).reshape(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    p = X @ R.T + np.asarray(tvec, dtype=np.float64).reshape(3)
    with np.errstate(all="ignore"):
        uv = p[:, :2] / p[:, 2:]
        if hasattr(camera, "world_to_image"):
            proj = np.asarray(camera.world_to_image(list(uv)), dtype=np.float64).reshape(-1, 2)
        else:
            proj = _world_to_image(camera.model_id, np.asarray(camera.params, dtype=np.float64), uv[:, 0], uv[:, 1])
        return list(np.linalg.norm(proj - p2D, axis=1))


def find_unique_inliers(idxs, pre_inliers=None):
    """main.py:38-47: the first (pre-)inlier of every index."""
    idxs = np.asarray(list(idxs))
    n = len(idxs)
    out = np.zeros(n, bool)
    if n == 0:
        return []
    pre = np.ones(n, bool) if pre_inliers is None else np.asarray(list(pre_inliers), dtype=bool)
    live = np.flatnonzero(pre)
    _, first = np.unique(idxs[live], return_index=True)
    out[live[first]] = True
    return [bool(x) for x in out]


def find_unique_min_by_group(errors, idxs, pre_inliers=None):
    """main.py:50-62: per index, the (pre-)inlier of smallest error (the first of equals)."""
    idxs, errors = np.asarray(list(idxs)), np.asarray(list(errors), dtype=np.float64)
    assert len(idxs) == len(errors)
    n = len(idxs)
    out = np.zeros(n, bool)
    if n == 0:
        return []
    pre = np.ones(n, bool) if pre_inliers is None else np.asarray(list(pre_inliers), dtype=bool)
    live = np.flatnonzero(pre)
    if len(live):
        _, group = np.unique(idxs[live], return_inverse=True)
        order = np.lexsort((live, errors[live], group))          # by group, then error, then position
        g = group[order]
        out[live[order[np.concatenate([[True], g[1:] != g[:-1]])]]] = True
    return [bool(x) for x in out]


def find_unique_min_reproj_inliers(pnp_points3D_id, qvec, tvec, camera, pnp_points2D, rec, pre_inliers=None, point2D_idxs=None):
    """main.py:65-77: one correspondence per 3D point, then one per keypoint, each the one of smallest reprojection error."""
    p3Ds = [rec.points3D[p3D_id] for p3D_id in pnp_points3D_id]
    errors = compute_reprojection_errors(pnp_points2D, p3Ds, qvec, tvec, camera)
    inliers = pre_inliers
    for idxs in [pnp_points3D_id, point2D_idxs]:
        if idxs is None:
            continue
        inliers = find_unique_min_by_group(errors, idxs, pre_inliers=inliers)
    return inliers


# ---- QueryLocalizer (main.py:261-537) ----------------------------------------------------------------------------------------------
_INHERIT = "${..interpolation}"


def _extractor_default_conf():
    from .extract import FeatureExtractor
    return deepcopy(FeatureExtractor.default_conf)


class QueryLocalizer:
    """pixsfm/localization/main.py:261-537.  Option 1: QueryLocalizer(reconstruction, conf, references=references); option 2:
    QueryLocalizer(reconstruction, conf, dense_features=feature_manager) extracts the references of every 3D point from the
    manager's feature sets; a Path for dense_features is read through the H5 cache reader if it exists.  Extracting (and
    caching) new map features is outside: the cache writer is."""

    default_conf = {
        "dense_features": _extractor_default_conf(),
        "overwrite_features_sparse": None,
        "interpolation": base.interpolation_default_conf,
        "target_reference": "nearest",
        "unique_inliers": "min_error",
        "references": {"loss": {"name": "cauchy", "params": [0.25]}, "iters": 100, "keep_observations": True,
                       "compute_offsets3D": False, "num_threads": -1},
        "max_tracks_per_problem": 50,
        "QKA": {**QueryKeypointAdjuster.default_conf, "interpolation": _INHERIT},
        "PnP": {"estimation": {"ransac": {"max_error": 12}}, "refinement": {}},
        "QBA": {**QueryBundleAdjuster.default_conf, "interpolation": _INHERIT},
    }

    def __init__(self, reconstruction, conf=None, dense_features=None, references=None, extractor=None, ctx=None):
        conf = deepcopy(dict(conf or {}))
        conf = conf.get("localization", conf)
        pnp = conf.pop("PnP", None) or {}
        dense = conf.pop("dense_features", None)
        merged = base.merge_conf({k: v for k, v in self.default_conf.items() if k not in ("PnP", "dense_features")}, conf)
        merged["dense_features"] = {**deepcopy(self.default_conf["dense_features"]), **(dense or {})}
        merged["PnP"] = {"estimation": {"ransac": {**self.default_conf["PnP"]["estimation"]["ransac"],
                                                   **((pnp.get("estimation") or {}).get("ransac") or {})},
                                        **{k: v for k, v in (pnp.get("estimation") or {}).items() if k != "ransac"}},
                         "refinement": dict(pnp.get("refinement") or {})}
        extra = set(pnp) - {"estimation", "refinement"}
        if extra:
            raise ValueError("unknown configuration key(s) %s in PnP" % sorted(extra))
        for part in ("QKA", "QBA"):                                # "${..interpolation}"
            if merged[part]["interpolation"] == _INHERIT:
                merged[part]["interpolation"] = deepcopy(merged["interpolation"])
        self.conf = merged
        abspose_engine_options(merged["PnP"]["estimation"], merged["PnP"]["refinement"])       # fail early on what PnP cannot take
        if merged["target_reference"] not in ("nearest", "robust_mean", "all_observations", "full"):
            raise ValueError("unknown target_reference %r" % (merged["target_reference"],))
        if merged["QKA"]["stack_correspondences"] and merged["target_reference"] not in ("nearest", "robust_mean"):
            raise ValueError("Stacked QKA requires a np.ndarray reference for each 2D-3D correspondence. Consider setting "
                             "target_references to 'nearest' or 'robust_mean'.")
        self.ctx = ctx
        self.query_keypoint_adjuster = QueryKeypointAdjuster(merged["QKA"], ctx=ctx)
        self.query_bundle_adjuster = QueryBundleAdjuster(merged["QBA"], ctx=ctx)
        self.extractor = extractor
        self.target_reference_funcs = {"nearest": self.get_nearest_references, "robust_mean": self.get_robust_mean_references,
                                       "all_observations": self.get_all_references, "full": self.get_full_references}
        self.get_query_references = self.target_reference_funcs[merged["target_reference"]]
        self.references = references
        self.reconstruction = reconstruction
        if self.references is None and (merged["QKA"]["apply"] or merged["QBA"]["apply"]):
            from .bundle_adjustment import ReferenceExtractor, find_problem_labels
            if isinstance(dense_features, (str, Path)):
                path = Path(dense_features)
                dense_features = features.load_features_from_cache(path, ctx=ctx) if path.exists() else None
            if dense_features is None:
                raise ValueError("QueryLocalizer needs `references` or the map's `dense_features` (a FeatureManager, or the path "
                                 "of an existing feature cache): extracting and caching new map features is outside the "
                                 "accelerated path (no cache writer)")
            self.reference_extractor = ReferenceExtractor(merged["references"], merged["interpolation"], ctx=ctx)
            labels = find_problem_labels(reconstruction, merged["max_tracks_per_problem"])
            self.references = [self.reference_extractor.run(labels, reconstruction, dense_features.fset(i))
                               for i in range(dense_features.num_levels)]

    def localize(self, keypoints, pnp_point2D_idxs, pnp_points3D_id, query_camera, image_path=None, query_fmaps=None,
                 return_covariance=False):
        """return_covariance: adds "covariance" to a successful result -- the 6 x 6 covariance of the final pose, (rotation in
        radians about the camera axes, translation), from the query bundle adjustment's problem at that pose (every point
        constant, residuals of unit variance).  Needs the features QKA / QBA work on."""
        assert len(pnp_point2D_idxs) == len(pnp_points3D_id)
        conf = self.conf
        require_feats = conf["QKA"]["apply"] or conf["QBA"]["apply"]
        assert image_path is not None or query_fmaps is not None or not require_feats
        if len(pnp_point2D_idxs) == 0:
            return {"success": False}
        pnp_point2D_idxs = [int(i) for i in pnp_point2D_idxs]
        pnp_points3D = [self.reconstruction.points3D[p3D_id].xyz for p3D_id in pnp_points3D_id]
        keypoints = np.array(keypoints, dtype=np.float64)

        # Extract Features
        if query_fmaps is None and require_feats:
            if self.extractor is None:
                from .extract import FeatureExtractor
                self.extractor = FeatureExtractor(conf["dense_features"], ctx=self.ctx)
            required_kp_ids = list(OrderedDict.fromkeys(pnp_point2D_idxs))
            query_fmaps = self.extractor(image_path, keypoints=keypoints[required_kp_ids], as_dict=False,
                                         keypoint_ids=required_kp_ids, overwrite_sparse=conf["overwrite_features_sparse"])

        # Get references for this query
        pnp_points2D = keypoints[pnp_point2D_idxs]
        query_references = None
        if require_feats:
            query_references = self.get_query_references(pnp_points3D_id, query_fmaps, pnp_points2D, pnp_point2D_idxs)
            assert len(query_fmaps) == len(query_references)

        # Run QKA
        if conf["QKA"]["apply"]:
            self.query_keypoint_adjuster.refine_multilevel(pnp_points2D, query_fmaps, query_references,
                                                           point2D_idxs=pnp_point2D_idxs)

        # Run PnP
        pose_dict = absolute_pose_estimation(pnp_points2D, pnp_points3D, query_camera,
                                             estimation_options=conf["PnP"]["estimation"],
                                             refinement_options=conf["PnP"]["refinement"], ctx=self.ctx)
        if not pose_dict["success"]:
            return pose_dict

        # For QBA we optionally select unique 2D-3D correspondences
        inliers = self._unique_inliers(pose_dict, pnp_points3D_id, query_camera, pnp_points2D, pnp_point2D_idxs)
        self.last_qba_inliers = list(inliers)

        # Run QBA
        if conf["QBA"]["apply"]:
            self.query_bundle_adjuster.refine_multilevel(pose_dict["qvec"], pose_dict["tvec"], query_camera, pnp_points3D,
                                                         query_fmaps, query_references, inliers=inliers,
                                                         point2D_idxs=pnp_point2D_idxs)

        if return_covariance:
            if not require_feats:
                raise ValueError("return_covariance needs the query's features: apply QKA or QBA, or pass query_fmaps")
            pose_dict["covariance"] = self.query_bundle_adjuster.covariance(pose_dict["qvec"], pose_dict["tvec"], query_camera,
                                                                            pnp_points3D, query_fmaps, query_references,
                                                                            inliers=inliers, point2D_idxs=pnp_point2D_idxs)

        # We recompute the inliers from the final pose
        errors = compute_reprojection_errors(pnp_points2D, pnp_points3D, pose_dict["qvec"], pose_dict["tvec"], query_camera)
        max_error = conf["PnP"]["estimation"]["ransac"]["max_error"]
        pose_dict["inliers"] = [bool(err < max_error) for err in errors]
        pose_dict["num_inliers"] = sum(pose_dict["inliers"])
        return pose_dict

    def _unique_inliers(self, pose_dict, pnp_points3D_id, query_camera, pnp_points2D, pnp_point2D_idxs):
        """The correspondences the QBA takes: PnP's inliers, made unique as conf["unique_inliers"] says (main.py:462-478)."""
        conf = self.conf
        inliers = pose_dict["inliers"]
        if conf["unique_inliers"]:                  # None and False: keep all
            if conf["unique_inliers"] == "random":
                inliers = find_unique_inliers(pnp_points3D_id, pre_inliers=inliers)
            elif conf["unique_inliers"] == "min_error":
                inliers = find_unique_min_reproj_inliers(pnp_points3D_id, pose_dict["qvec"], pose_dict["tvec"], query_camera,
                                                         pnp_points2D, self.reconstruction, pre_inliers=inliers,
                                                         point2D_idxs=pnp_point2D_idxs)
            else:
                import warnings
                warnings.warn("Unknown unique_inlier method %s." % (conf["unique_inliers"],))
        return inliers

    _BATCH_KEYS = ("keypoints", "pnp_point2D_idxs", "pnp_points3D_id", "query_camera", "image_path", "query_fmaps", "return_covariance")

    def localize_batch(self, queries):
        """localize() for many queries: `queries` is a list of dicts or tuples of localize()'s arguments (keypoints,
        pnp_point2D_idxs, pnp_points3D_id, query_camera, image_path=None, query_fmaps=None).  Per level the references of every
        query as in localize(), then ONE keypoint-adjustment launch over all queries per level, ONE absolute-pose launch, the
        unique inliers per query on the host, ONE bundle-adjustment launch per level over the queries PnP localized, and the final
        inlier recount.  Returns the list of localize()'s dicts: {"success": False} for a query without pairs, PnP's dict for one
        it could not localize.  Stacked correspondences and return_covariance are localize()'s: ValueError here."""
        conf = self.conf
        if conf["QKA"]["apply"] and conf["QKA"]["stack_correspondences"]:
            raise ValueError("localize_batch does not stack correspondences (QKA.stack_correspondences); call localize() per query")
        require_feats = conf["QKA"]["apply"] or conf["QBA"]["apply"]
        items = []
        for q in queries:
            if isinstance(q, dict):
                unknown = set(q) - set(self._BATCH_KEYS)
                if unknown:
                    raise ValueError("unknown argument(s) %s of a query" % sorted(unknown))
                a = dict(q)
            else:
                q = tuple(q)
                if not 4 <= len(q) <= len(self._BATCH_KEYS):
                    raise ValueError("a query is (keypoints, pnp_point2D_idxs, pnp_points3D_id, query_camera[, image_path[, query_fmaps]])")
                a = dict(zip(self._BATCH_KEYS, q))
            for k in ("keypoints", "pnp_point2D_idxs", "pnp_points3D_id", "query_camera"):
                if k not in a:
                    raise ValueError("a query needs %r" % (k,))
            if a.get("return_covariance"):
                raise ValueError("localize_batch does not return covariances (no batched covariance); call localize(..., "
                                 "return_covariance=True) per query")
            if len(a["pnp_point2D_idxs"]) != len(a["pnp_points3D_id"]):
                raise ValueError("pnp_point2D_idxs and pnp_points3D_id must have the same length")
            if require_feats and a.get("image_path") is None and a.get("query_fmaps") is None and len(a["pnp_point2D_idxs"]):
                raise ValueError("a query needs image_path or query_fmaps: QKA / QBA work on its features")
            items.append(a)

        out = [{"success": False} for _ in items]
        live = []
        for i, a in enumerate(items):
            if len(a["pnp_point2D_idxs"]) == 0:
                continue
            idxs = [int(k) for k in a["pnp_point2D_idxs"]]
            ids = list(a["pnp_points3D_id"])
            keypoints = np.array(a["keypoints"], dtype=np.float64)
            fmaps = a.get("query_fmaps")
            if fmaps is None and require_feats:                    # Extract Features
                if self.extractor is None:
                    from .extract import FeatureExtractor
                    self.extractor = FeatureExtractor(conf["dense_features"], ctx=self.ctx)
                required_kp_ids = list(OrderedDict.fromkeys(idxs))
                fmaps = self.extractor(a["image_path"], keypoints=keypoints[required_kp_ids], as_dict=False,
                                       keypoint_ids=required_kp_ids, overwrite_sparse=conf["overwrite_features_sparse"])
            p2D = keypoints[idxs]
            refs = None
            if require_feats:                                      # Get references for this query
                refs = self.get_query_references(ids, fmaps, p2D, idxs)
                assert len(fmaps) == len(refs)
            live.append(dict(i=i, idxs=idxs, ids=ids, p2D=p2D, p3D=[self.reconstruction.points3D[p].xyz for p in ids],
                             camera=a["query_camera"], fmaps=fmaps, refs=refs))
        if not live:
            return out

        if conf["QKA"]["apply"]:                                   # Run QKA: one launch per level
            n_levels = len(live[0]["fmaps"])
            if any(len(w["fmaps"]) != n_levels for w in live):
                raise ValueError("every query needs query_fmaps of the same %d levels" % n_levels)
            for level in resolve_level_indices(conf["QKA"]["level_indices"], n_levels):
                self.query_keypoint_adjuster.refine_batch([(w["p2D"], w["fmaps"][level], w["refs"][level], w["idxs"]) for w in live])

        poses = absolute_pose_estimation_batch([(w["p2D"], w["p3D"], w["camera"]) for w in live],       # Run PnP: one launch
                                               estimation_options=conf["PnP"]["estimation"],
                                               refinement_options=conf["PnP"]["refinement"], ctx=self.ctx)
        located = []
        for w, pose_dict in zip(live, poses):
            out[w["i"]] = pose_dict
            if pose_dict["success"]:
                w["pose"] = pose_dict
                w["inliers"] = self._unique_inliers(pose_dict, w["ids"], w["camera"], w["p2D"], w["idxs"])
                located.append(w)
        self.last_qba_inliers_batch = {w["i"]: list(w["inliers"]) for w in located}

        if conf["QBA"]["apply"] and located:                       # Run QBA: one launch per level
            self.query_bundle_adjuster.refine_multilevel_batch(
                [(w["pose"]["qvec"], w["pose"]["tvec"], w["camera"], w["p3D"], w["fmaps"], w["refs"], w["inliers"], w["idxs"])
                 for w in located])

        max_error = conf["PnP"]["estimation"]["ransac"]["max_error"]
        for w in located:                                          # We recompute the inliers from the final pose
            pose_dict = w["pose"]
            errors = compute_reprojection_errors(w["p2D"], w["p3D"], pose_dict["qvec"], pose_dict["tvec"], w["camera"])
            pose_dict["inliers"] = [bool(err < max_error) for err in errors]
            pose_dict["num_inliers"] = sum(pose_dict["inliers"])
        return out

    def get_nearest_references(self, pnp_points3D_id, query_fmaps, pnp_points2D, patch_idxs):
        return [find_nearest_references(query_fmaps[level], refs, pnp_points2D, pnp_points3D_id, self.conf["interpolation"],
                                        patch_idxs=patch_idxs, ctx=self.ctx) for level, refs in enumerate(self.references)]

    def get_robust_mean_references(self, pnp_points3D_id, *args):
        return [[np.asarray(refs[p3D_id].descriptor) for p3D_id in pnp_points3D_id] for refs in self.references]

    def get_all_references(self, pnp_points3D_id, *args):
        q_references = [[] for _ in self.references]
        for level, refs in enumerate(self.references):
            for p3D_id in pnp_points3D_id:
                if not refs[p3D_id].has_observations():
                    raise RuntimeError("Missing descriptors for observations.\nAssure that references.keep_observations==True.")
                q_references[level].append(list(refs[p3D_id].observations))
        return q_references

    def get_full_references(self, pnp_points3D_id, *args):
        raise NotImplementedError("target_reference 'full' feeds the patch-warp cost, which is outside the accelerated path; "
                                  "use 'nearest', 'robust_mean' or 'all_observations'")
