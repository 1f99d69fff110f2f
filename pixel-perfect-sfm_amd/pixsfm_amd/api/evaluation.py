"""Evaluation of a reconstruction: what the reference keeps in pixsfm/eval/eth3d.

Cloud accuracy and completeness (evaluate_point_cloud; triangulation.py:19-52 hands cloud and scan to ETH3D's
multi-view-evaluation program) run on the GPU: both directions are nearest-neighbour queries (pxr_cloud_nearest) followed by an
average over occupied voxels (pxr_cloud_voxel_fractions); DESIGN.md section 28.  Pose errors, recall and AUC
(localization.py:113-157), the similarity alignment of two reconstructions and PLY files are host code in float64: a scene has
thousands of images, not millions.

NOT MODELLED: the ETH3D program also takes occlusion and free-space meshes of the scan into account (points of the model that the
scanner could not have seen are left out of the accuracy).  Nothing of that is here, and parity with the program is unpinned."""
import numpy as np

from .. import engine
from .keypoint_adjustment import default_context
from .reconstruction import Reconstruction

_G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_MAX_DRAWS = 256
NUM_HYPOTHESES = 256       # three-centre samples of align_reconstructions
_SEED = 0                  # of their counter hash: fixed, the alignment is a function of its input alone


# ---- rotations -------------------------------------------------------------------------------------------------------------------
def _rotmat(qvec):
    w, x, y, z = np.asarray(qvec, dtype=np.float64) / np.linalg.norm(qvec)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _qvec(R):
    """Unit quaternion (w first, w >= 0) of a rotation matrix, by the largest of the four pivots."""
    t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
    k = int(np.argmax(t))
    d = 1.0 + t[k]
    if k == 0:
        q = np.array([d, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], d, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], d, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], d])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _centre(qvec, tvec):
    return -_rotmat(qvec).T @ np.asarray(tvec, dtype=np.float64)


# ---- pose errors, recall, AUC ----------------------------------------------------------------------------------------------------
def compute_pose_error(qvec_gt, tvec_gt, pose_dict):
    """(dt, dR) of an estimated pose {"success", "qvec", "tvec"} (world to camera) against the true one: the distance between the
    projection centres and the angle of the relative rotation in degrees; (inf, 180) for a pose that failed."""
    if not pose_dict.get("success", False):
        return np.inf, 180
    R_gt, R = _rotmat(qvec_gt), _rotmat(pose_dict["qvec"])
    dt = float(np.linalg.norm(_centre(qvec_gt, tvec_gt) - _centre(pose_dict["qvec"], pose_dict["tvec"])))
    cos = min(1.0, max(-1.0, (np.trace(R_gt @ R.T) - 1.0) / 2.0))
    return dt, float(np.degrees(np.arccos(cos)))


def compute_recall(errors):
    """The errors in ascending order and, for each, the fraction of all entries up to and including it."""
    e = np.sort(np.asarray(errors, dtype=np.float64).reshape(-1), kind="stable")
    return e, np.arange(1, len(e) + 1) / len(e)


def compute_auc(errors, thresholds, min_error=None):
    """Per threshold t: the area under the recall curve over [0, t], as a percentage of t.  The curve is the polygon through
    (0, 0) and the points of compute_recall, continued level from the last point at or below t up to t.  With min_error, every
    error at or below it counts as recalled from 0 on: the curve is level at their fraction over [0, min_error]."""
    e, r = compute_recall(errors)
    if min_error is None:
        x, y = np.concatenate([[0.0], e]), np.concatenate([[0.0], r])
    else:
        first = int(np.searchsorted(e, min_error, side="right"))
        level = first / len(e)
        x, y = np.concatenate([[0.0, float(min_error)], e[first:]]), np.concatenate([[level, level], r[first:]])
    out = []
    for t in thresholds:
        n = int(np.searchsorted(x, t, side="right"))                   # the points at or below t
        xs, ys = np.append(x[:n], t), np.append(y[:n], y[n - 1])
        area = float(np.sum(0.5 * (ys[1:] + ys[:-1]) * np.diff(xs)))
        out.append(area / t * 100.0)
    return out


# ---- similarity transforms -------------------------------------------------------------------------------------------------------
class Sim3:
    """x -> scale R(qvec) x + tvec."""

    def __init__(self, scale=1.0, qvec=(1.0, 0.0, 0.0, 0.0), tvec=(0.0, 0.0, 0.0)):
        self.scale = float(scale)
        self.qvec = np.array(qvec, dtype=np.float64)
        self.tvec = np.array(tvec, dtype=np.float64)

    @property
    def rotmat(self):
        return _rotmat(self.qvec)

    def transform_points(self, xyz):
        xyz = np.asarray(xyz, dtype=np.float64)
        return self.scale * xyz @ self.rotmat.T + self.tvec

    def inverse(self):
        R = self.rotmat
        return Sim3(1.0 / self.scale, _qvec(R.T), -(R.T @ self.tvec) / self.scale)

    def transform_pose(self, qvec, tvec):
        """The world-to-camera pose of a camera after its world went through this transform (camera coordinates keep the new
        world's unit: the centre moves with the points)."""
        R_new = _rotmat(qvec) @ self.rotmat.T
        return _qvec(R_new), -R_new @ self.transform_points(_centre(qvec, tvec))

    def transform_reconstruction(self, rec):
        """A copy of `rec` (cameras shared, observations kept) with poses and points in the transformed world."""
        from .reconstruction import Image, Point3D
        out = Reconstruction()
        out.cameras = dict(rec.cameras)
        for i, im in rec.images.items():
            q, t = self.transform_pose(im.qvec, im.tvec)
            out.add_image(Image(im.image_id, im.name, im.camera_id, q, t, im.points2D))
        for i, p in rec.points3D.items():
            out.add_point3D(i, Point3D(self.transform_points(p.xyz), p.track))
        return out

    def __repr__(self):
        return "Sim3(scale=%r, qvec=%r, tvec=%r)" % (self.scale, self.qvec.tolist(), self.tvec.tolist())


def _umeyama(src, dst):
    """The similarity (scale, R, t) with dst ~ scale R src + t in the least-squares sense (Umeyama 1991, eqs. 40-42), or None
    for a degenerate source (no spread)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    a, b = src - mu_s, dst - mu_d
    var = (a * a).sum() / len(src)
    if not var > 0:
        return None
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = (U * d) @ Vt
    scale = float((S * d).sum() / var)
    if not (np.isfinite(scale) and scale > 0):
        return None
    return scale, R, mu_d - scale * R @ mu_s


def _splitmix(z):
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _sample_three(seed, h, n):
    """Sample h of n >= 3 items: three distinct indices, ascending -- the counter hash of csrc/pxr_robust.h (sample_distinct<3>)
    restated: draw d = mix(mix(seed + G (h + 1)) + G d) mod n, a repeated index drawn again.  No random state."""
    a = _splitmix(seed + _G * (h + 1))
    draw = 0

    def nxt():
        nonlocal draw
        draw += 1
        return int(_splitmix(a + _G * draw) % n)
    c0 = nxt()
    c1 = nxt()
    while c1 == c0 and draw < _MAX_DRAWS:
        c1 = nxt()
    if c1 == c0:
        c1 = 1 if c0 == 0 else 0
    c2 = nxt()
    while c2 in (c0, c1) and draw < _MAX_DRAWS:
        c2 = nxt()
    if c2 in (c0, c1):
        c2 = 0 if (c0 != 0 and c1 != 0) else 1 if (c0 != 1 and c1 != 1) else 2
    return tuple(sorted((c0, c1, c2)))


def _centres_by_name(rec):
    return {im.name: _centre(im.qvec, im.tvec) for _, im in sorted(rec.images.items())}


def align_reconstructions(src, dst, max_error, min_inlier_ratio=0.3):
    """The similarity that takes `src` onto `dst`, fitted robustly to the projection centres of the images both hold (paired by
    name).  src / dst: Reconstructions, or {name: centre} dicts.  Returns (Sim3, inliers) with `inliers` a boolean mask over the
    common names in ascending order -- the order of compare_reconstructions(src, dst)["names"] -- or None with fewer than 3
    common images or fewer inliers than min_inlier_ratio of them.

    NUM_HYPOTHESES three-centre samples from the counter hash of csrc/pxr_robust.h (all triples where there are fewer), each a
    closed-form Umeyama fit; a centre is an inlier iff its squared error is <= max_error^2 (in dst's unit).  The best sample: most
    inliers, then the smaller sum of their squared errors, then the lower sample index.  Then at most 10 refits on the inliers,
    until the set stops changing; the mask returned is always that of the transform returned.  A function of the input alone."""
    a = src if isinstance(src, dict) else _centres_by_name(src)
    b = dst if isinstance(dst, dict) else _centres_by_name(dst)
    names = sorted(set(a) & set(b))
    n = len(names)
    if n < 3:
        return None
    A, B = np.array([a[k] for k in names], dtype=np.float64), np.array([b[k] for k in names], dtype=np.float64)
    thr2 = float(max_error) * float(max_error)

    def errors2(fit):
        s, R, t = fit
        d = s * A @ R.T + t - B
        return (d * d).sum(axis=1)

    n_triples = n * (n - 1) * (n - 2) // 6
    if n_triples <= NUM_HYPOTHESES:
        samples = [(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)]
    else:
        samples = [_sample_three(_SEED, h, n) for h in range(NUM_HYPOTHESES)]
    best, best_key = None, None
    for h, idx in enumerate(samples):
        fit = _umeyama(A[list(idx)], B[list(idx)])
        if fit is None:
            continue
        e2 = errors2(fit)
        inl = e2 <= thr2
        key = (-int(inl.sum()), float(e2[inl].sum()), h)
        if best_key is None or key < best_key:
            best, best_key = (fit, inl), key
    if best is None:
        return None
    fit, inl = best
    for _ in range(10):
        if inl.sum() < 3:
            break
        refit = _umeyama(A[inl], B[inl])
        if refit is None:
            break
        fit = refit
        fitted_to, inl = inl, errors2(fit) <= thr2                     # (inl is the mask of `fit` from here on)
        if np.array_equal(inl, fitted_to):
            break
    if inl.sum() < 3 or inl.sum() < min_inlier_ratio * n:
        return None
    return Sim3(fit[0], _qvec(fit[1]), fit[2]), inl


def compare_reconstructions(model, reference, sim3=None):
    """Pose and point differences of `model` against `reference` after `sim3` (None: identity) has been applied to the model.
    Returns {"names", "dt", "dR"} over the images both hold (by name, ascending; errors as compute_pose_error gives them, dR in
    degrees) and {"point3D_ids", "point_distances"} over the point ids both hold."""
    sim3 = sim3 or Sim3()
    ref_by_name = {im.name: im for im in reference.images.values()}
    names, dt, dR = [], [], []
    for im in sorted(model.images.values(), key=lambda im: im.name):
        if im.name not in ref_by_name:
            continue
        q, t = sim3.transform_pose(im.qvec, im.tvec)
        g = ref_by_name[im.name]
        e = compute_pose_error(g.qvec, g.tvec, {"success": True, "qvec": q, "tvec": t})
        names.append(im.name), dt.append(e[0]), dR.append(e[1])
    ids = sorted(set(model.points3D) & set(reference.points3D))
    dist = np.zeros(len(ids))
    if ids:
        moved = sim3.transform_points(np.array([model.points3D[i].xyz for i in ids]))
        dist = np.linalg.norm(moved - np.array([reference.points3D[i].xyz for i in ids]), axis=1)
    return {"names": names, "dt": np.array(dt), "dR": np.array(dR), "point3D_ids": ids, "point_distances": dist}


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
def _cloud(points):
    if isinstance(points, engine.DeviceArray):
        return points
    if hasattr(points, "points3D"):
        ids = sorted(points.points3D)
        return np.array([points.points3D[i].xyz for i in ids], dtype=np.float64).reshape(-1, 3)
    return np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)


def evaluate_point_cloud(points, scan, tolerances=(0.01, 0.02, 0.05), voxel_size=0.01, ctx=None):
    """Accuracy and completeness of a point cloud against a scan, per tolerance (the units of the clouds; the defaults are
    ETH3D's 1 / 2 / 5 cm).

    accuracy[t]: the fraction of `points` with a scan point within t; completeness[t]: the fraction of `scan` with a point within
    t -- both averaged over the occupied voxels of side voxel_size of the cloud that is asked about (0: over its points), so
    that a densely sampled surface does not outvote a sparsely sampled one.  points / scan: (n, 3) arrays, DeviceArrays, or a
    Reconstruction (its points3D in ascending id).  Returns {"tolerances", "accuracy", "completeness", "n_voxels"}: the dict of
    the reference's eval_multiview plus the voxel counts (points, scan).

    The ETH3D program's occlusion and free-space meshes are NOT modelled, and parity with it is unpinned (its source is not at
    hand): on a scan with large unobserved regions its accuracy is higher than this one's."""
    ctx = ctx or default_context()
    tol = [float(t) for t in tolerances]
    d_points = engine._device_cloud(ctx, _cloud(points), "points")
    d_scan = engine._device_cloud(ctx, _cloud(scan), "scan")
    reach = max(tol)
    _, d2 = engine.cloud_nearest(ctx, d_scan, d_points, reach)
    accuracy, n_points = engine.cloud_voxel_fractions(ctx, d_points, d2, voxel_size, tol)
    _, d2 = engine.cloud_nearest(ctx, d_points, d_scan, reach)
    completeness, n_scan = engine.cloud_voxel_fractions(ctx, d_scan, d2, voxel_size, tol)
    return {"tolerances": tol, "accuracy": [float(x) for x in accuracy], "completeness": [float(x) for x in completeness],
            "n_voxels": (n_points, n_scan)}


# ---- PLY -------------------------------------------------------------------------------------------------------------------------
def export_PLY(reconstruction_or_points, path, colors=None, binary=True):
    """Write vertices x y z as float32 (and red green blue as uchar when colours are given: `colors` (n, 3), or the `color` of a
    Reconstruction's points where they have one) to a PLY file, binary_little_endian by default."""
    src = reconstruction_or_points
    if hasattr(src, "points3D"):
        ids = sorted(src.points3D)
        xyz = np.array([src.points3D[i].xyz for i in ids], dtype=np.float64).reshape(-1, 3)
        if colors is None and ids and all(getattr(src.points3D[i], "color", None) is not None for i in ids):
            colors = np.array([src.points3D[i].color for i in ids])
    else:
        xyz = np.asarray(src.download() if isinstance(src, engine.DeviceArray) else src, dtype=np.float64).reshape(-1, 3)
    xyz = xyz.astype("<f4")
    if colors is not None:
        colors = np.asarray(colors).reshape(-1, 3).astype(np.uint8)
        if len(colors) != len(xyz):
            raise ValueError("colors must hold one row per point")
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(xyz),
            "property float x", "property float y", "property float z"]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            rec = np.zeros(len(xyz), dtype=[("p", "<f4", 3)] + ([("c", "u1", 3)] if colors is not None else []))
            rec["p"] = xyz
            if colors is not None:
                rec["c"] = colors
            f.write(rec.tobytes())
        else:
            for i in range(len(xyz)):
                row = ["%.9g" % v for v in xyz[i]] + ([str(int(c)) for c in colors[i]] if colors is not None else [])
                f.write((" ".join(row) + "\n").encode("ascii"))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_points(path, with_colors=False):
    """The vertices of a PLY file (ascii or binary_little_endian) as an (n, 3) float64 array of x y z; with_colors: also the
    (n, 3) uint8 red green blue, or None where the file has none.  Other vertex properties are skipped; list properties of the
    vertex element and big-endian files are not supported."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        fmt, n, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            w = line.decode("ascii", "replace").split()
            if not w or w[0] in ("comment", "obj_info"):
                continue
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                in_vertex = w[1] == "vertex"
                if in_vertex:
                    n = int(w[2])
                elif not props:
                    raise ValueError("%s: an element before the vertices is not supported" % path)
            elif w[0] == "property" and in_vertex:
                if w[1] == "list":
                    raise ValueError("%s: list properties of vertices are not supported" % path)
                props.append((w[2], _PLY_TYPES[w[1]]))
            elif w[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in "xyz"):
            raise ValueError("%s: vertices without x y z" % path)
        if fmt == "binary_little_endian":
            dt = np.dtype([(k, "<" + t) for k, t in props])
            data = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
            col = {k: data[k] for k in names}
        elif fmt == "ascii":
            rows = [f.readline().split() for _ in range(n)]
            col = {k: np.array([r[j] for r in rows], dtype=np.float64).astype(t) for j, (k, t) in enumerate(props)}
        else:
            raise ValueError("%s: format %s is not supported (ascii, binary_little_endian)" % (path, fmt))
    xyz = np.stack([np.asarray(col[k], dtype=np.float64) for k in "xyz"], axis=1).reshape(-1, 3)
    if not with_colors:
        return xyz
    rgb = ("red", "green", "blue")
    return xyz, (np.stack([col[k] for k in rgb], axis=1).astype(np.uint8) if all(k in names for k in rgb) else None)
