"""Track triangulation for the accelerated path: refined keypoints + track labels + known poses -> 3D points and tracks.

The reference hands this stage to COLMAP (PixSfM.triangulation -> hloc.triangulation.main -> pycolmap.triangulate_points,
pixsfm/refine_hloc.py:112-114); pycolmap is not installable where this library runs, so the stage is native here:
`TrackTriangulator.create(conf).triangulate(reconstruction, keypoints, graph)` takes what the keypoint adjustment returns
and produces the Reconstruction the bundle adjusters consume.  The estimator (pxr_triangulate_tracks)
enumerates two-view hypotheses in a fixed order and solves in ray space: reproducible bit for bit, no random state --
it is not COLMAP's sampler, and parity with COLMAP's triangulator is not pinned.
"""
import numpy as np

from ..engine import TriangulationProblem
from . import base
from .keypoint_adjustment import default_context
from .reconstruction import CAMERA_MODELS, Camera, Image, Point2D, Point3D, Reconstruction, Track

STATUS_NAMES = {0: "ok", 1: "too_few_observations", 2: "no_hypothesis", 3: "rejected"}


def flatten_tracks(reconstruction, keypoints, graph, track_labels):
    """The flat view of pxr_tri_view from pixsfm's objects (host logic, no GPU): images in ascending image id, cameras in
    ascending camera id, one track per track label in ascending label order, the nodes of a track in graph order.  Nodes with
    label -1, nodes whose image is not in the reconstruction and nodes without a keypoint entry are dropped.
    Returns the problem dict of engine.TriangulationProblem plus image_ids, camera_ids, track_label (per track) and
    obs_feature (per observation: the keypoint index in its image)."""
    if len(track_labels) != len(graph.nodes):
        raise ValueError("track_labels must have one entry per graph node")
    image_ids = sorted(reconstruction.images.keys())
    camera_ids = sorted(reconstruction.cameras.keys())
    cam_index = {c: i for i, c in enumerate(camera_ids)}
    index_of_name = {reconstruction.images[i].name: k for k, i in enumerate(image_ids)}
    cam_model = np.array([reconstruction.cameras[c].model_id for c in camera_ids], dtype=np.int32)
    cam_params = np.zeros((len(camera_ids), 12))
    for k, c in enumerate(camera_ids):
        cam = reconstruction.cameras[c]
        if int(cam.model_id) not in CAMERA_MODELS:
            raise ValueError("camera model id %d is not supported by the accelerated path" % cam.model_id)
        p = np.asarray(cam.params, dtype=np.float64)
        cam_params[k, :len(p)] = p
    images = [reconstruction.images[i] for i in image_ids]
    image_camera = np.array([cam_index[im.camera_id] for im in images], dtype=np.int32)
    qvec = np.array([im.qvec for im in images], dtype=np.float64).reshape(-1, 4)
    tvec = np.array([im.tvec for im in images], dtype=np.float64).reshape(-1, 3)

    labels = np.asarray(track_labels, dtype=np.int64)
    node_image = np.full(len(graph.nodes), -1, dtype=np.int64)
    node_feature = np.zeros(len(graph.nodes), dtype=np.int64)
    kps = {}
    for n, node in enumerate(graph.nodes):
        name = graph.image_id_to_name.get(node.image_id)
        k = index_of_name.get(name, -1)
        if k < 0 or name not in keypoints:
            continue
        if name not in kps:
            kps[name] = np.asarray(keypoints[name], dtype=np.float64).reshape(-1, 2)
        if not 0 <= node.feature_idx < len(kps[name]):
            raise ValueError("node %d names keypoint %d of %s, which has %d" % (n, node.feature_idx, name, len(kps[name])))
        node_image[n], node_feature[n] = k, node.feature_idx
    keep = np.flatnonzero((labels >= 0) & (node_image >= 0))
    keep = keep[np.argsort(labels[keep], kind="stable")]
    track_label, counts = np.unique(labels[keep], return_counts=True)
    offsets = np.zeros(len(track_label) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    obs_image = node_image[keep].astype(np.int32)
    obs_feature = node_feature[keep]
    obs_xy = np.empty((len(keep), 2))
    for i, (k, f) in enumerate(zip(obs_image, obs_feature)):
        obs_xy[i] = kps[images[k].name][f]
    return dict(track_offsets=offsets, obs_image=obs_image, obs_xy=obs_xy, image_camera=image_camera, qvec=qvec, tvec=tvec,
                cam_model=cam_model, cam_params=cam_params, image_ids=image_ids, camera_ids=camera_ids,
                track_label=track_label, obs_feature=obs_feature)


def build_reconstruction(reconstruction, keypoints, flat, xyz, status, obs_inlier):
    """A NEW Reconstruction: the cameras and posed images of `reconstruction`, every keypoint of every image as a point2D,
    one Point3D per track with status 0 (ids 1, 2, ... in track order) whose Track holds the final inliers only."""
    out = Reconstruction()
    for c in flat["camera_ids"]:
        cam = reconstruction.cameras[c]
        out.add_camera(Camera(c, int(cam.model_id), cam.width, cam.height, np.array(cam.params, dtype=np.float64)))
    for i in flat["image_ids"]:
        im = reconstruction.images[i]
        kp = np.asarray(keypoints.get(im.name, np.empty((0, 2))), dtype=np.float64).reshape(-1, 2)
        out.add_image(Image(i, im.name, im.camera_id, np.array(im.qvec), np.array(im.tvec), [Point2D(xy) for xy in kp]))
    offsets, image_ids = flat["track_offsets"], flat["image_ids"]
    point3D_of_track = {}
    for t in np.flatnonzero(np.asarray(status) == 0):
        pid = len(out.points3D) + 1
        track = Track()
        for o in range(offsets[t], offsets[t + 1]):
            if obs_inlier[o]:
                image_id, f = image_ids[flat["obs_image"][o]], int(flat["obs_feature"][o])
                track.add_element(image_id, f)
                out.images[image_id].points2D[f].point3D_id = pid
        out.add_point3D(pid, Point3D(xyz[t], track))
        point3D_of_track[int(t)] = pid
    return out, point3D_of_track


def mean_reprojection_error(ctx, reconstruction):
    """Mean pixel distance between the projection of every 3D point and the keypoints of its track (GPU, pxr_ba_geom_eval)."""
    from ..engine import GeometricBAProblem
    from .bundle_adjustment import BundleAdjustmentSetup, _FlatBA, _geometric_dict
    if not reconstruction.points3D:
        return float("nan")
    setup = BundleAdjustmentSetup()
    setup.add_images(reconstruction.reg_image_ids())
    flat = _FlatBA(reconstruction, setup, None, None, extractor=True)       # read-only: the quaternions stay as they are
    if len(flat.obs_image) == 0:
        return float("nan")
    return float(GeometricBAProblem(ctx, _geometric_dict(flat)).reprojection_errors().mean())


class TrackTriangulator:
    """Known poses in, points and tracks out -- in place of hloc.triangulation.main / pycolmap.triangulate_points."""
    default_conf = {
        'min_tri_angle': 1.5,        # degrees   } the values COLMAP's triangulator uses, which the reference inherits through hloc
        'max_angle_error': 2.0,      # degrees   }
        'max_reproj_error': 4.0,     # pixels    }
        'min_track_len': 2,
        'max_hypotheses': 256,       # two-view hypotheses per track (enumerated, not sampled)
        'refine': True,              # points-only geometric bundle adjustment afterwards, what triangulate_points ends with
    }

    def __init__(self, conf=None, ctx=None):
        self.conf = base.merge_conf(self.default_conf, conf)
        self.ctx = ctx

    @classmethod
    def create(cls, conf=None, ctx=None):
        return cls(conf, ctx)

    def options(self):
        return {k: self.conf[k] for k in ('min_tri_angle', 'max_angle_error', 'max_reproj_error', 'min_track_len', 'max_hypotheses')}

    def triangulate(self, reconstruction, keypoints, graph=None, track_labels=None):
        """reconstruction: cameras and posed images (ours or pycolmap's: same attribute names); keypoints {image name: (N, 2)}
        as the keypoint adjustment returns them; tracks from track_labels (one per graph node), or from the graph's labelling
        when absent.  Returns (a new Reconstruction, summary dict)."""
        if graph is None:
            raise ValueError("the match graph is needed: it says which keypoint of which image a track label belongs to")
        ctx = self.ctx or default_context()
        if track_labels is None:
            # the host labelling, or the device labelling (pxr_graph_gpu.hip) when the triangulator was given a context
            track_labels = base.compute_labels_on_device(graph, ctx)[0] if self.ctx is not None else base.compute_track_labels(graph)
        flat = flatten_tracks(reconstruction, keypoints, graph, track_labels)
        n_tracks = len(flat["track_label"])
        if n_tracks == 0:
            rec, _ = build_reconstruction(reconstruction, keypoints, flat, np.empty((0, 3)), np.empty(0, int), np.empty(0, np.uint8))
            return rec, {"num_tracks": 0, "num_points3D": 0, "status": {v: 0 for v in STATUS_NAMES.values()},
                         "mean_track_length": 0.0, "mean_reprojection_error": float("nan"), "refinement": None}
        problem = TriangulationProblem(ctx, flat)
        d_xyz, d_status, d_ninl, d_inl, d_err = problem.triangulate(**self.options())
        xyz, status, n_inl, inl, err = (a.download() for a in (d_xyz, d_status, d_ninl, d_inl, d_err))
        rec, point3D_of_track = build_reconstruction(reconstruction, keypoints, flat, xyz, status, inl)
        ok = status == 0
        summary = {
            "num_tracks": int(n_tracks), "num_points3D": int(ok.sum()),
            "status": {name: int((status == code).sum()) for code, name in STATUS_NAMES.items()},
            "mean_track_length": float(n_inl[ok].mean()) if ok.any() else 0.0,
            "mean_reprojection_error": float(err[inl.astype(bool)].mean()) if inl.any() else float("nan"),
            "refinement": None,
        }
        if self.conf['refine'] and ok.any():
            summary["refinement"] = self._refine_points(ctx, rec)
            summary["mean_reprojection_error_refined"] = mean_reprojection_error(ctx, rec)
        self.last = dict(flat=flat, xyz=xyz, status=status, n_inliers=n_inl, obs_inlier=inl, obs_err=err,
                         point3D_of_track=point3D_of_track)
        return rec, summary

    @staticmethod
    def _refine_points(ctx, rec):
        """The existing geometric bundle adjustment with every pose and every camera constant: only the points move.  Squared
        loss -- the tracks hold inliers only.  The solver hands back normalised quaternions (Image::NormalizeQvec); the
        triangulator's contract is poses in = poses out, so the input poses are put back as they were."""
        from .bundle_adjustment import BundleAdjustmentSetup, GeometricBundleOptimizer
        setup = BundleAdjustmentSetup()
        ids = rec.reg_image_ids()
        setup.add_images(ids)
        for i in ids:
            setup.set_constant_pose(i)
        for c in rec.cameras:
            setup.set_constant_camera(c)
        poses = {i: (rec.images[i].qvec.copy(), rec.images[i].tvec.copy()) for i in ids}
        cams = {c: rec.cameras[c].params.copy() for c in rec.cameras}
        options = {'loss': {'name': 'trivial', 'params': []}, 'solver': {'use_inner_iterations': False}, 'print_summary': False}
        solver = GeometricBundleOptimizer(options, setup, ctx=ctx)
        solver.run(rec)
        for i, (q, t) in poses.items():
            rec.images[i].qvec, rec.images[i].tvec = q, t
        for c, p in cams.items():
            rec.cameras[c].params = p
        return solver.summary()
