"""What the tests of incremental mapping share: the numpy reference of pxr_mapper_visibility (a direct transcription of the
semantics in include/pixsfm_hip.h), the boundary batch the kernel is held to, ring scenes with ground-truth tracks for the mapper,
and a similarity alignment for comparing its poses with ground truth."""
import functools

import numpy as np

from pixsfm_amd import synthetic

# visible observations per image: around the wavefront (64), the workgroup (256) and several passes of it (1025)
VISIBLE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
PARAMS = [1200.0, 500.0, 500.0, 0.02]          # SIMPLE_RADIAL, 1000 x 1000
# exact cell borders, the image corners and far outside, for a 640 x 480 image
BORDERS = ((0.0, 0.0), (640.0, 480.0), (320.0, 240.0), (-0.0, 479.999999), (639.9999999, 1e300), (-1e300, 10.0))


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def cell(x, levels, size):
    """clamp((int)floor(x 2^L / size), 0, 2^L - 1)"""
    return int(np.clip(np.floor(x * float(1 << levels) / float(size)), 0.0, float((1 << levels) - 1)))


def visibility_reference(scene, xyz, status, image_mask, levels):
    """scene: track_offsets, obs_image, obs_xy, image_camera, cam_size.  Returns the outputs of pxr_mapper_visibility with the
    correspondence arrays cut to n_corr rows."""
    off, obs_image, obs_xy = np.asarray(scene["track_offsets"]), np.asarray(scene["obs_image"]), np.asarray(scene["obs_xy"], dtype=np.float64)
    n_images, n_obs = len(scene["image_camera"]), len(obs_image)
    obs_track = np.repeat(np.arange(len(off) - 1), np.diff(off))
    n_visible, score = np.zeros(n_images, np.int32), np.zeros(n_images, np.int64)
    corr_obs, offsets = [], np.zeros(n_images + 1, np.int64)
    for i in range(n_images):
        if image_mask[i]:
            W, H = scene["cam_size"][scene["image_camera"][i]]
            cells = [set() for _ in range(levels + 1)]
            for o in range(n_obs):                                   # ascending observation order
                t = obs_track[o]
                if obs_image[o] != i or status[t] != 0 or not np.isfinite(xyz[t]).all() or not np.isfinite(obs_xy[o]).all():
                    continue
                corr_obs.append(o)
                n_visible[i] += 1
                cx, cy = cell(obs_xy[o, 0], levels, W), cell(obs_xy[o, 1], levels, H)
                for l in range(1, levels + 1):
                    cells[l].add((cx >> (levels - l), cy >> (levels - l)))
            score[i] = sum(4 ** l * len(cells[l]) for l in range(1, levels + 1))
        offsets[i + 1] = offsets[i] + n_visible[i]
    corr_obs = np.array(corr_obs, np.int64)
    return dict(n_visible=n_visible, score=score, corr_offsets=offsets, n_corr=int(offsets[-1]), corr_obs=corr_obs,
                corr_xy=obs_xy[corr_obs].reshape(-1, 2), corr_xyz=np.asarray(xyz, dtype=np.float64)[obs_track[corr_obs]].reshape(-1, 3))


# ---- the boundary batch ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_batch(seed=11):
    """One call that holds every case the kernel can get wrong.  Images 0 .. 8 have VISIBLE_COUNTS visible observations (plus
    invisible ones of every kind), image 9 is masked out although it sees points, image 10 sees only tracks without a point:
    11 images.  Two cameras of different size alternate.  Keypoints reach 20 % outside the image on every side (the cells
    clamp); image 4 sees one track twice.  Returns (scene, xyz, status, image_mask, planned visible counts)."""
    rng = np.random.default_rng(seed)
    cam_size = np.array([[640, 480], [1000, 750]], np.int32)
    n_images = len(VISIBLE_COUNTS) + 2
    image_camera = (np.arange(n_images) % 2).astype(np.int32)
    n_good, n_nopoint, n_nanxyz = 1400, 60, 20
    n_tracks = n_good + n_nopoint + n_nanxyz
    status = np.zeros(n_tracks, np.int32)
    status[n_good:n_good + n_nopoint] = rng.integers(1, 4, n_nopoint)
    xyz = rng.uniform(-1, 1, (n_tracks, 3))
    xyz[n_good:n_good + n_nopoint] = np.nan                          # what a track without a point holds
    xyz[n_good + n_nopoint:, rng.integers(0, 3, n_nanxyz)] = np.nan  # status 0, yet no finite point
    xyz[n_good + n_nopoint, :] = np.inf
    obs = []                                                         # (track, image, x, y)

    def pixel(i):
        W, H = cam_size[image_camera[i]]
        return rng.uniform(-0.2 * W, 1.2 * W), rng.uniform(-0.2 * H, 1.2 * H)

    planned = np.zeros(n_images, np.int64)
    for i in range(n_images):
        v = VISIBLE_COUNTS[i] if i < len(VISIBLE_COUNTS) else (300 if i == len(VISIBLE_COUNTS) else 0)
        tracks = rng.permutation(n_good)[:v - len(BORDERS) if i == 2 else v]
        if i == 4:
            tracks[-1] = tracks[0]                                   # one track seen twice by this image
        for t in tracks:
            obs.append((t, i) + pixel(i))
        planned[i] = v if i != len(VISIBLE_COUNTS) else 0            # (image 9 is masked out)
        for t in n_good + rng.permutation(n_nopoint + n_nanxyz)[:17 if i != 1 else 0]:
            obs.append((t, i) + pixel(i))
        for t in rng.permutation(n_good)[:5 if i not in (0, 1) else 0]:   # a good track, a keypoint that is not finite
            x, y = pixel(i)
            obs.append((t, i) + ((np.nan, y) if t % 2 else (x, np.inf)))
    for x, y in BORDERS:                                             # on image 2 (640 x 480), among its 63 visible ones
        obs.append((int(rng.integers(n_good)), 2, x, y))
    obs = np.array(obs, dtype=np.float64)
    order = np.lexsort((rng.permutation(len(obs)), obs[:, 0]))       # track-major, images in no order inside a track
    obs = obs[order]
    track = obs[:, 0].astype(np.int64)
    offsets = np.zeros(n_tracks + 1, np.int64)
    np.cumsum(np.bincount(track, minlength=n_tracks), out=offsets[1:])
    scene = dict(track_offsets=offsets, obs_image=obs[:, 1].astype(np.int32), obs_xy=np.ascontiguousarray(obs[:, 2:4]),
                 image_camera=image_camera, cam_model=np.array([2, 2], np.int32),
                 cam_params=np.array([[600.0, 320.0, 240.0, 0.01], [900.0, 500.0, 375.0, 0.0]]), cam_size=cam_size)
    mask = np.ones(n_images, np.uint8)
    mask[len(VISIBLE_COUNTS)] = 0
    mask[2] = 7                                                      # any non-zero value is a candidate
    return scene, xyz, status, mask, planned


@functools.lru_cache(maxsize=None)
def many_images_batch(n_images):
    """Many images with a handful of observations each (0 .. 4, a fifth of them on tracks without a point), every tenth image
    masked out: what the prefix sum over the images' counts can get wrong around the size of its workgroup (256 threads: 255, 256,
    257 images, and 600 -- three images to a thread).  Returns (scene, xyz, status, image_mask)."""
    rng = np.random.default_rng(n_images)
    cam_size = np.array([[640, 480]], np.int32)
    n_tracks = 40
    status = np.zeros(n_tracks, np.int32)
    status[32:] = 1
    xyz = rng.uniform(-1, 1, (n_tracks, 3))
    xyz[32:] = np.nan
    per_image = rng.integers(0, 5, n_images)
    image = np.repeat(np.arange(n_images), per_image)
    track = rng.integers(0, n_tracks, len(image))
    order = np.lexsort((rng.permutation(len(image)), track))         # track-major, images in no order inside a track
    offsets = np.zeros(n_tracks + 1, np.int64)
    np.cumsum(np.bincount(track, minlength=n_tracks), out=offsets[1:])
    scene = dict(track_offsets=offsets, obs_image=image[order].astype(np.int32), obs_xy=rng.uniform(0.0, 480.0, (len(image), 2)),
                 image_camera=np.zeros(n_images, np.int32), cam_model=np.array([2], np.int32),
                 cam_params=np.array([[600.0, 320.0, 240.0, 0.01]]), cam_size=cam_size)
    mask = np.ones(n_images, np.uint8)
    mask[::10] = 0
    return scene, xyz, status, mask


def bad_inputs(scene):
    """(name, key of the device array to replace, the bad host array, a word of the message) for every class of bad input."""
    off, n_obs = np.asarray(scene["track_offsets"]), len(scene["obs_image"])
    n_images, n_tracks = len(scene["image_camera"]), len(off) - 1
    from pixsfm_amd.engine import image_major_transpose
    io, iobs = image_major_transpose(scene["obs_image"], n_images)
    obs_track = np.repeat(np.arange(n_tracks, dtype=np.int64), np.diff(off))

    def put(a, k, v):
        a = np.array(a)
        a[k] = v
        return a
    swapped = put(put(iobs, io[4], iobs[io[4] + 1]), io[4] + 1, iobs[io[4]])        # image 4's first two entries, descending
    return [
        ("track offsets not monotone", "track_offsets", put(off, 5, off[6] + 1), "monotone"),
        ("track offsets not ending at n_obs", "track_offsets", put(off, n_tracks, n_obs - 1), "n_obs"),
        ("image offsets not monotone", "image_obs_offsets", put(io, 3, io[4] + 1), "monotone"),
        ("image offsets not ending at n_obs", "image_obs_offsets", put(io, n_images, n_obs + 1), "n_obs"),
        ("track index too large", "obs_track", put(obs_track, 17, n_tracks), "track"),
        ("track index negative", "obs_track", put(obs_track, n_obs - 1, -1), "track"),
        ("observation index out of range", "image_obs", put(iobs, 40, n_obs), "observation"),
        ("image_obs not ascending", "image_obs", swapped, "transpose"),
        ("observation filed under another image", "obs_image", put(scene["obs_image"], 0, (scene["obs_image"][0] + 1) % n_images), "transpose"),
        ("image index out of range", "obs_image", put(scene["obs_image"], 3, n_images), "transpose"),
        ("camera index out of range", "image_camera", put(scene["image_camera"], 2, 2), "camera"),
        ("camera size not positive", "cam_size", put(scene["cam_size"], (1, 0), 0), "width"),
    ]


# ---- scenes for the mapper ---------------------------------------------------------------------------------------------------------
def ring_scene(n_images=10, n_points=300, views=6, sigma=0.5, seed=0, n_images_second=0, unmatched=0, cocentred=False,
               wrong_share=0.0):
    """Ring cameras looking at a cloud of points, each point seen by `views` neighbouring images, keypoints with Gaussian noise
    sigma, ONE SIMPLE_RADIAL camera object for all images, tracks from ground truth.
      n_images_second  a second ring of that many images around a second cloud far away: a disconnected component
      unmatched        that many further images whose keypoints belong to no track
      cocentred        one more image at the centre of image 0, rotated by 20 degrees, seeing ALL points of image 0 (and more of
                       the cloud): with image 0 it forms the pair of most matches, and it has no parallax
      wrong_share      this share of the track members is reassigned to another track (the keypoint stays where it is)
    Returns dict(cameras, keypoints, names, owner {name: point per keypoint, -1 none}, label_of {name: track label per keypoint},
    wrong {name: bool per keypoint}, poses {name: (qvec, tvec)}, X)."""
    from pixsfm_amd.api.reconstruction import Camera
    rng = np.random.default_rng(seed)
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    rings = [(n_images, np.zeros(3), 0)]
    if n_images_second:
        rings.append((n_images_second, np.array([500.0, 0.0, 0.0]), n_images))
    names, poses, kps, owner = [], {}, {}, {}
    X_all = []
    for n_ring, centre, first_image in rings:
        qvec, tvec = synthetic.ring_cameras(n_ring, rng=rng)
        tvec = np.array([t - synthetic.qvec_to_rotmat(q) @ centre for q, t in zip(qvec, tvec)])
        ring_names = ["image%02d.jpg" % (first_image + i) for i in range(n_ring)]
        for i, nm in enumerate(ring_names):
            names.append(nm); poses[nm] = (qvec[i], tvec[i]); kps[nm] = []; owner[nm] = []
        n_pts = n_points if first_image == 0 else max(n_points // 3, 1)     # fewer matches per pair than in the first ring
        X = rng.uniform(-1, 1, (n_pts, 3)) + centre
        base_point = len(X_all)
        X_all.extend(X)
        for p in range(n_pts):
            first = rng.integers(n_ring)
            for j in range(min(views, n_ring)):
                nm = ring_names[(first + j) % n_ring]
                kps[nm].append(synthetic.project(2, PARAMS, *poses[nm], X[p]) + rng.normal(0, sigma, 2))
                owner[nm].append(base_point + p)
    if cocentred:
        q0, t0 = poses[names[0]]
        R0 = synthetic.qvec_to_rotmat(q0)
        a = np.radians(20.0)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])      # about the optical axis
        nm = "image%02d.jpg" % len(names)
        names.append(nm); poses[nm] = (synthetic.rotmat_to_qvec(Rz @ R0), Rz @ t0); kps[nm] = []; owner[nm] = []
        seen0 = set(owner[names[0]])
        for p in range(n_points):
            if p in seen0 or p % 2 == 0:
                kps[nm].append(synthetic.project(2, PARAMS, *poses[nm], X_all[p]) + rng.normal(0, sigma, 2))
                owner[nm].append(p)
    for k in range(unmatched):
        nm = "image%02d.jpg" % len(names)
        names.append(nm); poses[nm] = (np.array([1.0, 0, 0, 0]), np.zeros(3))
        kps[nm] = list(rng.uniform(0, 1000, (50, 2))); owner[nm] = [-1] * 50
    label_of, wrong = {}, {}
    n_all = len(X_all)
    for nm in names:
        kps[nm] = np.array(kps[nm], dtype=np.float64).reshape(-1, 2)
        owner[nm] = np.array(owner[nm], dtype=np.int64)
        label_of[nm] = owner[nm].copy()
        wrong[nm] = np.zeros(len(owner[nm]), bool)
        if wrong_share > 0:
            pick = (rng.uniform(size=len(owner[nm])) < wrong_share) & (owner[nm] >= 0)
            label_of[nm][pick] = (owner[nm][pick] + 1 + rng.integers(0, n_all - 1, pick.sum())) % n_all
            wrong[nm] = pick
    return dict(cameras={nm: camera for nm in names}, keypoints=kps, names=names, owner=owner, label_of=label_of, wrong=wrong,
                poses=poses, X=np.array(X_all), camera=camera)


WRONG_SEED = 5      # of the scene with members of wrong tracks: the seed (of 0 .. 11) with the largest wrong_member_clearance, 19.5 px


def wrong_member_clearance(scene):
    """The smallest pixel distance between a keypoint that was put into a wrong track and the true projection of that track's
    point into its image.  A wrong member closer than the widest inlier threshold of the pipeline (12 px, absolute pose) is a
    member that no geometric test can tell from a right one: a scene for the trap must stay clear of that."""
    best = np.inf
    for nm in scene["names"]:
        q, t = scene["poses"][nm]
        for f in np.flatnonzero(scene["wrong"][nm]):
            best = min(best, np.linalg.norm(synthetic.project(2, PARAMS, q, t, scene["X"][scene["label_of"][nm][f]]) - scene["keypoints"][nm][f]))
    return float(best)


def matches_from_labels(scene):
    """All pairs of images that share track labels: (pairs, matches) with one match per shared label (the first keypoint of
    that label in either image)."""
    names, label_of = scene["names"], scene["label_of"]
    first = {}
    for nm in names:
        lab = label_of[nm]
        uniq, idx = np.unique(lab[lab >= 0], return_index=True)
        first[nm] = (uniq, np.flatnonzero(lab >= 0)[idx])
    pairs, matches = [], []
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            (la, ia), (lb, ib) = first[names[a]], first[names[b]]
            common, ka, kb = np.intersect1d(la, lb, return_indices=True)
            if len(common):
                pairs.append((names[a], names[b]))
                matches.append(np.stack([ia[ka], ib[kb]], 1))
    return pairs, matches


def graph_and_labels(scene, pairs, matches):
    """The match graph of these matches and the track label of every node from the scene's labelling."""
    from pixsfm_amd.api import build_matching_graph
    graph = build_matching_graph(pairs, matches, [np.ones(len(m)) for m in matches])
    labels = [int(scene["label_of"][graph.image_id_to_name[node.image_id]][int(node.feature_idx)]) for node in graph.nodes]
    return graph, labels


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
def umeyama(src, dst):
    """The similarity (s, R, t) with dst ~ s R src + t in the least-squares sense (Umeyama 1991)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    a, b = src - mu_s, dst - mu_d
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (a ** 2).sum() * len(src)
    return s, R, mu_d - s * R @ mu_s


def pose_errors(rec, poses):
    """Rotation (degrees) and centre errors of the images of `rec` against ground-truth poses {name: (qvec, tvec)}, after the
    similarity alignment of the camera centres.  Returns (max rotation error, max centre error)."""
    q2r = synthetic.qvec_to_rotmat
    ims = [rec.images[i] for i in sorted(rec.images)]
    c_est = np.array([-q2r(im.qvec).T @ im.tvec for im in ims])
    c_gt = np.array([-q2r(poses[im.name][0]).T @ poses[im.name][1] for im in ims])
    s, R, t = umeyama(c_est, c_gt)
    rot, cen = [], []
    for im, ce, cg in zip(ims, c_est, c_gt):
        dR = q2r(im.qvec) @ R.T @ q2r(poses[im.name][0]).T            # estimated world -> gt world, then compare camera frames
        rot.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
        cen.append(np.linalg.norm(s * R @ ce + t - cg))
    return float(max(rot)), float(max(cen))
