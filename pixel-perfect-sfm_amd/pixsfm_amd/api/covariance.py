"""Uncertainty of a bundle adjustment: what `pycolmap.estimate_ba_covariance` / COLMAP's EstimateBACovariance /
`ceres::Covariance` give on the CPU, computed by pxr_ba_covariance from the solver's own linearisation on the GPU.

    cov = estimate_ba_covariance({"strategy": "geometric"}, reconstruction)
    cov.pose_cov(image_id)          # 6 x 6, (rotation in radians about the camera axes, translation)
    cov.point_cov(point3D_id)       # 3 x 3

The problem -- which images, cameras and points take part, and what is constant -- is the bundle adjusters' own: the optimizers'
`set_up` builds it, so a covariance belongs to exactly the problem a refinement with the same configuration solves.
"""
import numpy as np

from .. import _lib
from ..engine import make_loss
from . import base

ROT_TO_RADIANS = 2.0          # the solver's rotation tangent is the half-angle vector of QuaternionManifold::Plus


def half_angle_to_radians(block):
    """A 6 x 6 pose block in the solver's units (half-angle rotation tangent, translation) in (radians, translation): the
    rotation block times 4, the rotation-translation blocks times 2."""
    s = np.array([ROT_TO_RADIANS] * 3 + [1.0] * 3)
    return np.asarray(block, dtype=np.float64) * s[:, None] * s[None, :]


def posterior_factor(cost, num_residuals, num_parameters):
    """sigma^2 of the residuals estimated from the fit, 2 cost / (m - n): what scale="posterior" multiplies by."""
    dof = int(num_residuals) - int(num_parameters)
    if dof <= 0:
        raise ValueError("scale='posterior' needs more residuals (%d) than parameters (%d)" % (num_residuals, num_parameters))
    return 2.0 * float(cost) / dof


def rank_deficiency_message(summary, columns, image_ids, camera_ids):
    """The text of the ValueError for a reduced camera matrix that is rank deficient (summary["info"] > 0)."""
    col, n_c = int(summary["info"]) - 1, int(summary["num_camera_unknowns"])
    where = "column %d" % col
    for k, (off, dim) in enumerate(zip(columns["pose_off"], columns["pose_dim"])):
        if off <= col < off + dim:
            where = "the pose of image %s" % (image_ids[k],)
    for k, (off, dim) in enumerate(zip(columns["intr_off"], columns["intr_dim"])):
        if off <= col < off + dim:
            where = "the intrinsics of camera %s" % (camera_ids[k],)
    free_poses = sum(1 for d in columns["pose_dim"] if d == 6)
    return ("the gauge is not fixed: the reduced camera matrix is rank deficient at column %d of %d (%s); %d camera-side columns "
            "were free, %d of %d poses without any constant component -- hold one pose constant and one more translation "
            "component (BundleAdjustmentSetup.set_constant_pose / set_constant_tvec) before asking for a covariance"
            % (col + 1, n_c, where, n_c, free_poses, len(columns["pose_dim"])))


class BACovariance:
    """Blocks of the covariance of a bundle adjustment, by COLMAP id.  Rotations are in radians about the camera axes
    (pose_cov, cameras_cov); intrinsics in the units of the camera parameters; points in scene units.  Rows and columns of
    constant parameters are zero."""

    def __init__(self, image_ids, camera_ids, point_ids, cam_model, cov, factor=1.0, cost=None, num_residuals=None,
                 num_parameters=None):
        self.image_ids, self.camera_ids, self.point_ids = list(image_ids), list(camera_ids), list(point_ids)
        self._img = {i: k for k, i in enumerate(self.image_ids)}
        self._cam = {c: k for k, c in enumerate(self.camera_ids)}
        self._pt = {p: k for k, p in enumerate(self.point_ids)}
        self._model = [int(m) for m in cam_model]
        self._cov, self.factor = cov, float(factor)
        self.summary = dict(cov["summary"], cost=cost, num_residuals=num_residuals, num_parameters=num_parameters, factor=self.factor)

    def pose_cov(self, image_id):
        if image_id not in self._img:
            raise KeyError("image %r is not part of the problem" % (image_id,))
        return half_angle_to_radians(self._cov["pose"][self._img[image_id]]) * self.factor

    def intrinsics_cov(self, camera_id):
        if camera_id not in self._cam:
            raise KeyError("camera %r is not part of the problem" % (camera_id,))
        k = self._cam[camera_id]
        n = _lib.CAMERA_NUM_PARAMS[self._model[k]]
        return self._cov["intrinsics"][k][:n, :n] * self.factor

    def point_cov(self, point3D_id):
        if point3D_id not in self._pt:
            raise KeyError("point %r is not part of the problem" % (point3D_id,))
        return self._cov["points"][self._pt[point3D_id]] * self.factor

    def cameras_cov(self):
        """(Sigma_c (n_c, n_c), columns): the dense covariance of all camera-side unknowns and, per column, ("pose", image_id,
        component 0..5 of (rotation, translation)) or ("intrinsics", camera_id, parameter index)."""
        cols = self._cov["columns"]
        names, scale = [], []
        for k, slots in enumerate(cols["pose_slots"]):
            names += [("pose", self.image_ids[k], s) for s in slots]
            scale += [ROT_TO_RADIANS if s < 3 else 1.0 for s in slots]
        for k, slots in enumerate(cols["intr_slots"]):
            names += [("intrinsics", self.camera_ids[k], s) for s in slots]
            scale += [1.0] * len(slots)
        s = np.asarray(scale, dtype=np.float64)
        return self._cov["cameras"] * s[:, None] * s[None, :] * self.factor, names


def _optimizer_for(conf, setup):
    from . import bundle_adjustment as ba
    strategy = conf.get("strategy", "feature_reference")
    options = conf.get("optimizer")
    interpolation = conf.get("interpolation")
    if strategy == "geometric":
        return ba.GeometricBundleOptimizer(options, setup)
    if strategy == "feature_reference":
        return ba.FeatureReferenceBundleOptimizer(options, setup, interpolation)
    if strategy == "costmaps":
        return ba.CostMapBundleOptimizer(options, setup, dict(interpolation or base.interpolation_default_conf, l2_normalize=False))
    raise ValueError("strategy %r is outside the accelerated path (feature_reference, costmaps, geometric)" % (strategy,))


def estimate_ba_covariance(optimizer_or_conf, reconstruction, problem_setup=None, feature_view=None, references=None, scale="unit"):
    """Covariance of the poses, intrinsics and points of `reconstruction` at its current parameters.

    optimizer_or_conf: a bundle optimizer that has not been set up yet (GeometricBundleOptimizer,
    FeatureReferenceBundleOptimizer, CostMapBundleOptimizer), or the configuration of a BundleAdjuster (`strategy`,
    `optimizer`, `interpolation`) together with problem_setup (default: default_problem_setup).  feature_view: the feature set
    or view of `feature_reference` (with `references`) or the cost-map view of `costmaps`; nothing for `geometric`.
    scale: "unit" -- inv(J^T J), residuals of unit variance -- or "posterior": times 2 cost / (m - n).
    Raises ValueError when the gauge is not fixed."""
    from . import bundle_adjustment as ba
    if scale not in ("unit", "posterior"):
        raise ValueError("scale must be 'unit' or 'posterior'")
    if isinstance(optimizer_or_conf, dict) or optimizer_or_conf is None:
        setup = problem_setup if problem_setup is not None else ba.default_problem_setup(reconstruction)
        optimizer = _optimizer_for(dict(optimizer_or_conf or {}), setup)
    else:
        optimizer = optimizer_or_conf
        if problem_setup is not None and problem_setup is not optimizer.setup:
            raise ValueError("an optimizer brings its own problem setup")
    if isinstance(optimizer, ba.GeometricBundleOptimizer):
        optimizer.set_up(reconstruction, None)
    elif isinstance(optimizer, ba.CostMapBundleOptimizer):
        optimizer.set_up(reconstruction, None, feature_view)
    else:
        optimizer.set_up(reconstruction, None, feature_view, references)
    try:
        flat, problem = optimizer._flat, optimizer._ba
        if problem is None:
            raise ValueError("the problem has no residuals")
        if getattr(optimizer, "_share", None) is not None:
            raise ValueError("estimate_ba_covariance runs on one rank")
        loss = make_loss(optimizer._loss['name'], optimizer._loss['params'])
        if isinstance(optimizer, ba.GeometricBundleOptimizer):
            problem.eval(residuals=False)
        else:
            problem.eval(optimizer.interpolation.to_engine(), with_jacobian=True)
        cost = problem.cost(loss)
        cov = problem.covariance(loss, flat.pose_const, flat.tvec_mask, flat.cam_mask, flat.point_const, cameras=True)
        if cov["summary"]["info"] != 0:
            raise ValueError(rank_deficiency_message(cov["summary"], cov["columns"], flat.image_ids, flat.camera_ids))
        variable = int(np.count_nonzero(np.asarray(flat.point_const) == 0)) - int(cov["summary"]["num_singular_points"])
        m = len(flat.obs_image) * optimizer._residuals_per_observation()
        n = int(cov["summary"]["num_camera_unknowns"]) + 3 * variable
        factor = posterior_factor(cost, m, n) if scale == "posterior" else 1.0
        return BACovariance(flat.image_ids, flat.camera_ids, flat.point_ids, flat.cam_model, cov, factor, cost, m, n)
    finally:
        optimizer.reset()
