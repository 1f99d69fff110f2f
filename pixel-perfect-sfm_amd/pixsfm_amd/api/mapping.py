"""Incremental mapping for the accelerated path: verified matches in, poses and points out.

The reference's main entry point PixSfM.reconstruction (pixsfm/refine_hloc.py:133-146) hands this stage to hloc.reconstruction.main,
i.e. COLMAP's incremental mapper; pycolmap is not installable where this library runs, so the stage is native here:
`IncrementalMapper.create(conf).reconstruct(cameras, keypoints, graph, pairs, geometries)` takes what the keypoint adjustment and
TwoViewVerifier / TwoViewClassifier return and produces the Reconstruction the bundle adjusters consume.

This is a BATCHED-ROUND mapper, not COLMAP's one-image-at-a-time order: every round triangulates all tracks
over the registered images, runs one global geometric bundle adjustment, triangulates again from the refined poses, ranks ALL
unregistered images on the device (pxr_mapper_visibility) and registers the candidates in ONE pxr_absolute_pose launch.  It is
deterministic and has no random state.  The defaults are COLMAP's IncrementalMapper::Options as remembered; parity with COLMAP is
not pinned.  Out of scope: several models per scene, local bundle adjustment, track merging / completion, scene normalisation,
uncalibrated initialisation, COLMAP database / model files.
"""
import time

import numpy as np

from ..engine import (AbsolutePoseProblem, GeometricBAProblem, MapperScene, TriangulationProblem, _padded_cam_params, lm_options,
                      make_loss)
from ..synthetic import qvec_to_rotmat
from . import base
from .bundle_adjustment import linear_solver_for
from .keypoint_adjustment import default_context
from .reconstruction import CAMERA_MODELS, Camera, Image, Point2D, Point3D, Reconstruction, Track
from .triangulation import TrackTriangulator, flatten_tracks

INIT_CONFIGS = ("CALIBRATED", "PLANAR")


def initial_pair_order(geometries, max_trials):
    """The pair indices tried as the initial pair: geometries with `success` (and, where a `config` is given, one of CALIBRATED /
    PLANAR), by (num_inliers descending, pair index ascending), at most max_trials of them."""
    cand = [p for p, g in enumerate(geometries)
            if g.get("success") and (g.get("config") is None or g["config"] in INIT_CONFIGS)]
    cand.sort(key=lambda p: (-int(geometries[p]["num_inliers"]), p))
    return cand[:max(int(max_trials), 0)]


def gauge_component(tvec):
    """The component of the second image's translation that the bundle adjustment holds constant: the one of largest magnitude
    (the first of equals)."""
    return int(np.argmax(np.abs(np.asarray(tvec, dtype=np.float64))))


def median_triangulation_angle(xyz, centre1, centre2):
    """The median over the points of the angle (degrees) under which the two centres are seen (host numpy)."""
    if len(xyz) == 0:
        return 0.0
    a, b = xyz - centre1, xyz - centre2
    cos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return float(np.median(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))))


# -- the stages both mappers share (IncrementalMapper here, GlobalMapper in global_mapping.py), on flat arrays -----------------------
def triangulate_registered(conf, st, registered):
    """Tracks restricted to the registered images -> (problem, restricted dict, device outputs), or None without observations."""
    r = st["scene"].restricted_tracks(registered)
    if len(r["obs_index"]) == 0:
        return None
    prob = TriangulationProblem(st["ctx"], dict(track_offsets=r["track_offsets"], obs_image=r["obs_image"], obs_xy=r["obs_xy"],
                                                image_camera=st["image_camera"], qvec=st["qvec"], tvec=st["tvec"],
                                                cam_model=st["cam_model"], cam_params=st["cam_params"]))
    out = prob.triangulate(timed=True, **conf['triangulation'])
    st["ms"]["triangulate"] += sum(prob.kernel_ms.values())
    return prob, r, out


def retriangulate(conf, st, prob):
    """The same tracks again from the poses (and intrinsics) of st."""
    prob.d["qvec"].upload(st["qvec"])
    prob.d["tvec"].upload(st["tvec"])
    prob.d["cam_params"].upload(_padded_cam_params(st["cam_params"], len(st["cam_model"])))
    out = prob.triangulate(timed=True, **conf['triangulation'])
    st["ms"]["triangulate"] += sum(prob.kernel_ms.values())
    return out


def bundle_adjust(conf, st, registered, r, out):
    """Global geometric bundle adjustment with trivial loss over the registered images and the tracks with a point: the
    first image of st["init"] constant, the translation component st["gauge"] of the second constant.  Poses (and intrinsics, if
    refined) of st are updated.  Returns (GeometricBAProblem, summary, flat index arrays) or None when there is no point."""
    d_xyz, d_status, _, d_inl, _ = out
    status, inl, xyz = d_status.download(), d_inl.download().astype(bool), d_xyz.download()
    sel = np.flatnonzero(inl)
    if len(sel) == 0:
        return None
    obs_track = np.repeat(np.arange(len(status), dtype=np.int64), np.diff(r["track_offsets"]))
    images = np.flatnonzero(registered)
    points = np.flatnonzero(status == 0)
    cams = np.unique(st["image_camera"][images])
    img_new = np.full(len(registered), -1, np.int32); img_new[images] = np.arange(len(images), dtype=np.int32)
    pt_new = np.full(len(status), -1, np.int32); pt_new[points] = np.arange(len(points), dtype=np.int32)
    cam_new = np.full(len(st["cam_model"]), -1, np.int32); cam_new[cams] = np.arange(len(cams), dtype=np.int32)
    obs_image = img_new[r["obs_image"][sel]]
    ba = GeometricBAProblem(st["ctx"], dict(obs_image=obs_image, obs_point=pt_new[obs_track[sel]], obs_xy=r["obs_xy"][sel],
                                            image_camera=cam_new[st["image_camera"][images]], qvec=st["qvec"][images],
                                            tvec=st["tvec"][images], cam_model=st["cam_model"][cams],
                                            cam_params=st["cam_params"][cams], xyz=xyz[points]))
    pose_const = np.zeros(len(images), np.uint8)
    pose_const[np.bincount(obs_image, minlength=len(images)) == 0] = 1          # an image all of whose observations were filtered
    pose_const[img_new[st["init"][0]]] = 1
    tvec_mask = np.zeros(len(images), np.uint8)
    tvec_mask[img_new[st["init"][1]]] = 1 << st["gauge"]
    cam_mask = np.zeros(len(cams), np.uint16)
    for k, c in enumerate(cams):
        _, n_params, focal, _, _ = CAMERA_MODELS[int(st["cam_model"][c])]
        mask = (1 << n_params) - 1
        if conf['ba_refine_focal_length']:
            for a in focal:
                mask &= ~(1 << a)
        cam_mask[k] = mask
    opts = lm_options(max_iterations=int(conf['ba_max_num_iterations']), linear_solver=linear_solver_for(len(images)))
    t0 = time.perf_counter()
    summ = ba.solve(make_loss("trivial", []), pose_const, tvec_mask, cam_mask, np.zeros(len(points), np.uint8), options=opts)
    st["ms"]["bundle_adjustment_wall"] += 1e3 * (time.perf_counter() - t0)
    q, t, k, _ = ba.params()
    st["qvec"][images], st["tvec"][images] = q, t
    st["cam_params"][cams] = k[:, :st["cam_params"].shape[1]]
    return ba, summ, dict(sel=sel, obs_track=obs_track, images=images, points=points)


def finish(conf, st, skeleton, flat, keypoints, registered, summary):
    """The end of a reconstruction: triangulate over the registered images, adjust, filter by reprojection error, and build the
    Reconstruction of the registered images with the tracks that keep two observations.  Fills final_ba,
    num_filtered_observations, mean_reprojection_error, num_reg_images and num_points3D of `summary`."""
    prob, r, out = triangulate_registered(conf, st, registered)
    done = bundle_adjust(conf, st, registered, r, out)
    rec = Reconstruction()
    for k, c in enumerate(flat["camera_ids"]):
        cam = skeleton.cameras[c]
        rec.add_camera(Camera(c, int(cam.model_id), cam.width, cam.height, st["cam_params"][k, :len(cam.params)].copy()))
    for k in np.flatnonzero(registered):
        im = skeleton.images[flat["image_ids"][k]]
        kp = np.asarray(keypoints[im.name], dtype=np.float64).reshape(-1, 2)
        rec.add_image(Image(im.image_id, im.name, im.camera_id, st["qvec"][k].copy(), st["tvec"][k].copy(), [Point2D(xy) for xy in kp]))
    if done is not None:
        ba, summ, ix = done
        err = ba.reprojection_errors()
        xyz = ba.params()[3]
        keep = err <= float(conf['filter_max_reproj_error'])
        point_of_obs = np.searchsorted(ix["points"], ix["obs_track"][ix["sel"]])
        length = np.bincount(point_of_obs[keep], minlength=len(ix["points"]))
        obs_full = r["obs_index"][ix["sel"]]
        pid_of_point = np.full(len(ix["points"]), -1, np.int64)
        for j in np.flatnonzero(length >= 2):
            pid_of_point[j] = len(rec.points3D) + 1
            rec.add_point3D(int(pid_of_point[j]), Point3D(xyz[j], Track()))
        for o, j in zip(obs_full[keep], point_of_obs[keep]):
            if pid_of_point[j] < 0:
                continue
            image_id, f = flat["image_ids"][flat["obs_image"][o]], int(flat["obs_feature"][o])
            rec.points3D[int(pid_of_point[j])].track.add_element(image_id, f)
            rec.images[image_id].points2D[f].point3D_id = int(pid_of_point[j])
        kept = keep & (pid_of_point[point_of_obs] >= 0)
        summary.update(final_ba=summ, num_filtered_observations=int((~keep).sum()),
                       mean_reprojection_error=float(err[kept].mean()) if kept.any() else float("nan"))
    summary.update(num_reg_images=int(registered.sum()), num_points3D=len(rec.points3D))
    return rec


class IncrementalMapper:
    """Verified matches in, registered images and points out -- in place of hloc.reconstruction.main / COLMAP's mapper."""
    default_conf = {
        'init_min_num_inliers': 100,
        'init_min_tri_angle': 16.0,          # degrees
        'init_max_trials': 20,
        'abs_pose_max_error': 12.0,          # pixels
        'abs_pose_min_num_inliers': 30,
        'abs_pose_min_inlier_ratio': 0.25,
        'max_reg_trials': 3,
        'max_images_per_round': 0,           # 0 = all candidates of a round
        'pyramid_levels': 6,
        'filter_max_reproj_error': 4.0,      # pixels
        'ba_max_num_iterations': 50,
        'ba_refine_focal_length': False,
        'triangulation': {k: v for k, v in TrackTriangulator.default_conf.items() if k != 'refine'},
    }

    def __init__(self, conf=None, ctx=None):
        self.conf = base.merge_conf(self.default_conf, conf)
        c = self.conf
        if not 1 <= int(c['pyramid_levels']) <= 6:
            raise ValueError("pyramid_levels must be in [1, 6]")
        for k in ('init_min_num_inliers', 'init_max_trials', 'abs_pose_min_num_inliers', 'max_reg_trials', 'ba_max_num_iterations'):
            if int(c[k]) < 1:
                raise ValueError("%s must be at least 1" % k)
        if int(c['max_images_per_round']) < 0:
            raise ValueError("max_images_per_round must be 0 (all) or positive")
        for k in ('abs_pose_max_error', 'filter_max_reproj_error'):
            if not float(c[k]) > 0.0:
                raise ValueError("%s must be positive" % k)
        if not 0.0 <= float(c['abs_pose_min_inlier_ratio']) <= 1.0:
            raise ValueError("abs_pose_min_inlier_ratio must be in [0, 1]")
        if not 0.0 <= float(c['init_min_tri_angle']) < 180.0:
            raise ValueError("init_min_tri_angle must be in [0, 180)")
        self.ctx = ctx

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: a dict over default_conf; unknown keys raise ValueError."""
        return cls(conf, ctx)

    # -- the one walk over the input objects ---------------------------------------------------------------------------------
    @staticmethod
    def _skeleton(cameras, keypoints):
        """A Reconstruction of unposed images (ids 1, 2, ... in the order of `cameras`) over the distinct camera objects."""
        rec, cam_id = Reconstruction(), {}
        for k, (name, cam) in enumerate(cameras.items()):
            if name not in keypoints:
                raise KeyError("no keypoints for image %r" % (name,))
            if int(cam.model_id) not in CAMERA_MODELS:
                raise ValueError("camera model id %d is not supported by the accelerated path" % cam.model_id)
            if id(cam) not in cam_id:
                cam_id[id(cam)] = len(cam_id) + 1
                rec.add_camera(Camera(cam_id[id(cam)], int(cam.model_id), cam.width, cam.height, np.array(cam.params, dtype=np.float64)))
            rec.add_image(Image(k + 1, name, cam_id[id(cam)], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0]))
        return rec

    # -- the stages of a round that are the mapper's own (the shared ones are the module's functions above) ------------------
    def _register(self, st, registered, trials, d_xyz, d_status):
        """Visibility of the unregistered images that have trials left, then one absolute-pose launch over the candidates.
        Returns (number of candidates, indices of the newly registered images)."""
        c, scene, ctx = self.conf, st["scene"], st["ctx"]
        mask = ~registered & (trials < int(c['max_reg_trials']))
        if not mask.any():
            return 0, []
        vis = scene.visibility(d_xyz, d_status, mask, int(c['pyramid_levels']), timed=True)
        st["ms"]["visibility"] += sum(scene.kernel_ms.values())
        n_visible, score = vis["n_visible"].download(), vis["score"].download()
        cand = np.flatnonzero(mask & (n_visible >= int(c['abs_pose_min_num_inliers'])))
        cand = cand[np.lexsort((cand, -score[cand]))]                              # (score descending, image index ascending)
        if int(c['max_images_per_round']) > 0:
            cand = cand[:int(c['max_images_per_round'])]
        if len(cand) == 0:
            return 0, []
        chosen = np.zeros(len(mask), bool); chosen[cand] = True
        if not np.array_equal(chosen, mask):                                        # only the candidates become queries
            vis = scene.visibility(d_xyz, d_status, chosen, int(c['pyramid_levels']), timed=True)
            st["ms"]["visibility"] += sum(scene.kernel_ms.values())
        scene.d["cam_params"].upload(_padded_cam_params(st["cam_params"], len(st["cam_model"])))
        pose = AbsolutePoseProblem.from_device(ctx, vis["corr_offsets"], vis["n_corr"], vis["corr_xy"], vis["corr_xyz"],
                                               scene.d["image_camera"], scene.d["cam_model"], scene.d["cam_params"])
        d_q, d_t, d_st, d_ni, _, _, _ = pose.estimate(timed=True, max_error=float(c['abs_pose_max_error']),
                                                     min_num_inliers=int(c['abs_pose_min_num_inliers']),
                                                     min_inlier_ratio=float(c['abs_pose_min_inlier_ratio']))
        st["ms"]["absolute_pose"] += sum(pose.kernel_ms.values())
        q, t, status, n_inl = d_q.download(), d_t.download(), d_st.download(), d_ni.download()
        new = []
        for i in cand:
            ok = status[i] == 0 and n_inl[i] >= int(c['abs_pose_min_num_inliers']) \
                and n_inl[i] >= float(c['abs_pose_min_inlier_ratio']) * n_visible[i]
            if ok:
                registered[i] = True
                st["qvec"][i], st["tvec"][i] = q[i], t[i]
                new.append(int(i))
            else:
                trials[i] += 1
        return len(cand), new

    def _initialise(self, st, pairs, geometries, index_of_name):
        """The first pair that triangulates enough points under enough parallax: (pair index, registered mask) or (None, None)."""
        c, n = self.conf, len(st["image_camera"])
        for p in initial_pair_order(geometries, c['init_max_trials']):
            a, b = index_of_name.get(pairs[p][0]), index_of_name.get(pairs[p][1])
            if a is None or b is None or a == b:
                continue
            g = geometries[p]
            t = np.asarray(g["tvec"], dtype=np.float64)
            if not np.linalg.norm(t) > 0.0:
                continue
            registered = np.zeros(n, bool); registered[[a, b]] = True
            st["qvec"][:], st["tvec"][:] = [1.0, 0.0, 0.0, 0.0], 0.0
            st["qvec"][b], st["tvec"][b] = np.asarray(g["qvec"], dtype=np.float64), t / np.linalg.norm(t)
            tri = triangulate_registered(self.conf, st, registered)
            if tri is None:
                continue
            d_xyz, d_status = tri[2][0], tri[2][1]
            xyz = d_xyz.download()[d_status.download() == 0]
            centre2 = -qvec_to_rotmat(st["qvec"][b]).T @ st["tvec"][b]
            angle = median_triangulation_angle(xyz, np.zeros(3), centre2)
            st["init_trials"].append(dict(pair=tuple(pairs[p]), num_points=int(len(xyz)), median_tri_angle=angle))
            if len(xyz) >= int(c['init_min_num_inliers']) and angle >= float(c['init_min_tri_angle']):
                st["init"], st["gauge"] = (a, b), gauge_component(st["tvec"][b])
                return p, registered
        return None, None

    def reconstruct(self, cameras, keypoints, graph, pairs, geometries, track_labels=None):
        """cameras {image name: camera} (calibrated; images that share a camera object share its intrinsics), keypoints {image
        name: (N, 2)}, the match graph after verification, pairs [(name1, name2)] and geometries as TwoViewVerifier /
        TwoViewClassifier return them (success, qvec, tvec, num_inliers, optional config); tracks from track_labels (one per graph
        node), or from the graph's labelling when absent.  Returns (Reconstruction of the registered images, summary dict)."""
        pairs, geometries = list(pairs), list(geometries)
        if len(pairs) != len(geometries):
            raise ValueError("pairs and geometries must have the same length")
        ctx = self.ctx or default_context()
        skeleton = self._skeleton(cameras, keypoints)
        if track_labels is None:
            track_labels = base.compute_track_labels(graph)
        flat = flatten_tracks(skeleton, keypoints, graph, track_labels)
        names = [skeleton.images[i].name for i in flat["image_ids"]]
        index_of_name = {n: k for k, n in enumerate(names)}
        cam_size = np.array([[skeleton.cameras[c].width, skeleton.cameras[c].height] for c in flat["camera_ids"]], np.int32).reshape(-1, 2)
        n = len(names)
        st = dict(ctx=ctx, image_camera=flat["image_camera"], cam_model=flat["cam_model"], cam_params=flat["cam_params"].copy(),
                  qvec=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), tvec=np.zeros((n, 3)), init_trials=[],
                  ms=dict(triangulate=0.0, visibility=0.0, absolute_pose=0.0, bundle_adjustment_wall=0.0))
        summary = dict(status="no_initial_pair", initial_pair=None, num_reg_images=0, unregistered=list(names), rounds=[],
                       num_points3D=0, init_trials=st["init_trials"], kernel_ms=st["ms"])
        if n < 2 or len(flat["obs_image"]) == 0:
            return Reconstruction(), summary
        st["scene"] = MapperScene(ctx, dict(flat, cam_size=cam_size))
        t0 = time.perf_counter()
        p0, registered = self._initialise(st, pairs, geometries, index_of_name)
        summary["init_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if p0 is None:
            return Reconstruction(), summary
        summary["status"], summary["initial_pair"] = "ok", tuple(pairs[p0])
        trials = np.zeros(n, np.int64)
        while True:
            before, t0 = dict(st["ms"]), time.perf_counter()
            prob, r, out = triangulate_registered(self.conf, st, registered)
            done = bundle_adjust(self.conf, st, registered, r, out)
            if done is not None:
                out = retriangulate(self.conf, st, prob)
            n_points = int((out[1].download() == 0).sum())
            n_cand, new = self._register(st, registered, trials, out[0], out[1])
            ms = {k: st["ms"][k] - before[k] for k in before}
            ms["round_wall"] = 1e3 * (time.perf_counter() - t0)
            summary["rounds"].append(dict(candidates=n_cand, registered=len(new), points=n_points,
                                          ba=None if done is None else done[1], ms=ms))
            if not new:
                break
        rec = finish(self.conf, st, skeleton, flat, keypoints, registered, summary)
        summary.update(unregistered=[names[k] for k in np.flatnonzero(~registered)])
        return rec, summary
