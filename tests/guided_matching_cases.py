"""The guided matcher's reference, written from the specification (include/pixsfm_hip.h, pxr_match_guided)
and not from the kernels: `admissible` in numpy float64 with exactly the operation order of the header, then the unguided
reference of tests/matching_cases.py over the similarity matrix with every inadmissible entry replaced by NaN.  A second
statement of the same rules (`guided_reference_loops`: per-row Python loops over the admissible columns) checks the first.
The generators of the test cases follow, all with fixed seeds."""
import numpy as np

import matching_cases as mc

EPIPOLAR, HOMOGRAPHY = 0, 1          # PXR_GUIDE_EPIPOLAR, PXR_GUIDE_HOMOGRAPHY
KINDS = {"epipolar": EPIPOLAR, "homography": HOMOGRAPHY}


def admissible(kind, M, thr, xy_a, xy_b):
    """(na, nb) bool: which (i, j) the model admits.  float64, one rounding per operation, in the order of the header."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    xy_a, xy_b = np.asarray(xy_a, np.float64).reshape(-1, 2), np.asarray(xy_b, np.float64).reshape(-1, 2)
    if not np.all(np.isfinite(M)):                     # a model that is not finite admits nothing
        return np.zeros((len(xy_a), len(xy_b)), dtype=bool)
    x, y, u, v = xy_a[:, 0], xy_a[:, 1], xy_b[:, 0], xy_b[:, 1]
    thr = np.float64(thr)
    with np.errstate(all="ignore"):
        if kind == EPIPOLAR:
            l0 = (M[0, 0] * x + M[0, 1] * y) + M[0, 2]
            l1 = (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
            l2 = (M[2, 0] * x + M[2, 1] * y) + M[2, 2]
            ra = l0 * l0 + l1 * l1
            m0 = (M[0, 0] * u + M[1, 0] * v) + M[2, 0]
            m1 = (M[0, 1] * u + M[1, 1] * v) + M[2, 1]
            cb = m0 * m0 + m1 * m1
            t = (u[None, :] * l0[:, None] + v[None, :] * l1[:, None]) + l2[:, None]
            den = ra[:, None] + cb[None, :]
            return (den > 0) & (t * t <= (thr * thr) * den)
        if kind == HOMOGRAPHY:
            X = (M[0, 0] * x + M[0, 1] * y) + M[0, 2]
            Y = (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
            Wd = (M[2, 0] * x + M[2, 1] * y) + M[2, 2]
            px, py = X / Wd, Y / Wd
            dx, dy = px[:, None] - u[None, :], py[:, None] - v[None, :]
            return (Wd > 0)[:, None] & (dx * dx + dy * dy <= thr * thr)
    raise ValueError("unknown kind %r" % (kind,))


def guided_reference(A, B, xy_a, xy_b, kind, M, thr, **options):
    """(matches0, scores0, n_matches) of one pair: an inadmissible entry is a NaN similarity."""
    adm = admissible(kind, M, thr, xy_a, xy_b)
    return mc.match_from_sim(np.where(adm, mc.sim_chain(A, B), np.float32(np.nan)).astype(np.float32), **options)


def _loop_side(sim, adm, r2, t2, skip):
    f = np.float32
    out, s1s = np.full(sim.shape[0], -1, np.int32), np.full(sim.shape[0], -np.inf, f)
    for i in range(sim.shape[0]):
        cand = [j for j in range(sim.shape[1]) if adm[i, j] and not np.isnan(sim[i, j])]
        if not cand:
            continue
        s1 = max(sim[i, j] for j in cand)
        best = min(j for j in cand if sim[i, j] == s1)
        s2 = max([sim[i, j] for j in cand if j != best], default=f(-np.inf))
        s1s[i] = s1
        with np.errstate(all="ignore"):
            d1, d2 = f(2) * (f(1) - f(s1)), f(2) * (f(1) - f(s2))
            if r2 is not None and not skip and not d1 <= r2 * d2:
                continue
            if t2 is not None and not d1 <= t2:
                continue
        out[i] = best
    return out, s1s


def guided_reference_loops(A, B, xy_a, xy_b, kind, M, thr, ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True):
    """The same rules stated a second way: per row (and per column) a Python loop over the admissible candidates with max."""
    f = np.float32
    sim, adm = mc.sim_chain(A, B), admissible(kind, M, thr, xy_a, xy_b)
    r2 = f(ratio_threshold * ratio_threshold) if ratio_threshold > 0 else None
    t2 = f(distance_threshold * distance_threshold) if distance_threshold > 0 else None
    skip = sim.shape[0] == 1 or sim.shape[1] == 1
    m0, s1 = _loop_side(sim, adm, r2, t2, skip)
    if do_mutual_check:
        m1, _ = _loop_side(np.ascontiguousarray(sim.T), np.ascontiguousarray(adm.T), r2, t2, skip)
        for i in range(len(m0)):
            if m0[i] >= 0 and m1[m0[i]] != i:
                m0[i] = -1
    scores = np.array([(s + f(1)) / f(2) if m >= 0 else f(0) for m, s in zip(m0, s1)], dtype=f).reshape(-1)
    return m0, scores, int((m0 >= 0).sum())


def reference_batch(descs, xy, pairs, kinds, models, thrs, options=None):
    """The flat outputs of pxr_match_guided: matches0, scores0, n_matches, pair_offsets."""
    options = options or mc.CONFS["NN-mutual"]
    res = [guided_reference(descs[a], descs[b], xy[a], xy[b], kinds[p], models[p], thrs[p], **options) for p, (a, b) in enumerate(pairs)]
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in res])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.empty(0, dt)   # noqa: E731
    return cat(0, np.int32), cat(1, np.float32), np.array([r[2] for r in res], dtype=np.int32), off


# ---- generators -------------------------------------------------------------------------------------------------------------------
def _error(kind, M, xy_a, xy_b):
    """The squared error of every entry in the units of thr^2 (plain numpy, for choosing thresholds only)."""
    xa, xb = np.c_[xy_a, np.ones(len(xy_a))], np.c_[xy_b, np.ones(len(xy_b))]
    with np.errstate(all="ignore"):
        if kind == EPIPOLAR:
            la, lb = xa @ M.T, xb @ M
            return (xb @ la.T).T ** 2 / ((la[:, 0] ** 2 + la[:, 1] ** 2)[:, None] + (lb[:, 0] ** 2 + lb[:, 1] ** 2)[None, :])
        p = xa @ M.T
        return ((p[:, :2] / p[:, 2:])[:, None, :] - xy_b[None, :, :]).__pow__(2).sum(-1)


def threshold_for(kind, M, xy_a, xy_b, fraction):
    """The threshold under which about `fraction` of the entries are admissible (1.0 where there is no finite entry)."""
    e = _error(kind, M, xy_a, xy_b)
    e = e[np.isfinite(e)]
    return float(np.sqrt(np.quantile(e, fraction))) if e.size else 1.0


def random_model(rng, kind):
    """A random rank-2 matrix (epipolar) or a random near-identity homography."""
    if kind == EPIPOLAR:
        U, s, Vt = np.linalg.svd(rng.standard_normal((3, 3)))
        return (U * np.array([s[0], s[1], 0.0])) @ Vt
    H = np.eye(3) + 0.1 * rng.standard_normal((3, 3))
    H[2, :2] *= 0.3                                   # Wd stays positive over [-1, 1]^2
    return H


def consistent_keypoints(rng, kind, M, xy_b):
    """Per keypoint of image b a keypoint of image a that the model maps onto it (up to 1e-3 of noise)."""
    n = len(xy_b)
    xb = np.c_[xy_b, np.ones(n)]
    if kind == EPIPOLAR:                              # a random point, projected onto the line M^t x_b of image a
        line = xb @ M
        p = rng.uniform(-1, 1, (n, 2))
        d = (line[:, 0] * p[:, 0] + line[:, 1] * p[:, 1] + line[:, 2]) / (line[:, 0] ** 2 + line[:, 1] ** 2)
        out = p - d[:, None] * line[:, :2]
    else:
        q = xb @ np.linalg.inv(M).T
        out = q[:, :2] / q[:, 2:]
    return out + 1e-3 * rng.standard_normal((n, 2))


def gated_pair(na, nb, dim, kind, seed, shared=0.6, fraction=0.2):
    """matching_cases.pair_case plus keypoints in [-1, 1]^2, a random model of `kind` and a threshold that admits about a fifth
    of the entries; the keypoints of the shared descriptors are consistent with the model, so that matches survive.
    Returns dict(A, B, xy_a, xy_b, kind, M, thr)."""
    A, B = mc.pair_case(na, nb, dim, seed, shared=shared)
    replay = np.random.default_rng(seed)              # pair_case's own draws, to learn which rows it shared
    mc.unit_rows(replay, na, dim), mc.unit_rows(replay, nb, dim)
    k = int(shared * min(na, nb))
    ia, ib = replay.permutation(na)[:k], replay.permutation(nb)[:k]
    rng = np.random.default_rng(seed + 7919)
    M = random_model(rng, kind)
    xy_a, xy_b = rng.uniform(-1, 1, (na, 2)), rng.uniform(-1, 1, (nb, 2))
    xy_a[ia] = consistent_keypoints(rng, kind, M, xy_b[ib])
    return dict(A=A, B=B, xy_a=xy_a, xy_b=xy_b, kind=kind, M=M, thr=threshold_for(kind, M, xy_a, xy_b, fraction))


def edge_pair(kind, dim=128, seed=41):
    """48 x 64 descriptors whose admissibility is planted through the keypoints: a keypoint sits in a `band`, and (i, j) is
    admissible iff both sit in the same band.  Epipolar: E of a pure x translation, for which x_b^t E x_a = y_a - v_b, keypoints
    (0, band); homography: M = [[1, 0, 0], [0, 1, 0], [-1, 0, 1]] (Wd = 1 - x), keypoints (0, band).  Planted:
      row 3 / column 9     a band of their own: no admissible partner
      row 7 - column 21    a band of their own: exactly one admissible partner, kept under NN-ratio
      row 12               its unguided best (column 30, a bit-identical copy) is inadmissible; the runner-up (column 32) wins
      row 11               three bit-identical admissible copies at columns 5, 17, 40: the lowest wins
      row 20 / column 33   a NaN keypoint
      rows 24, 25          (homography) Wd = 0 and Wd < 0
    Returns dict(A, B, xy_a, xy_b, kind, M, thr)."""
    rng = np.random.default_rng(seed)
    na, nb = 48, 64
    A, B = mc.unit_rows(rng, na, dim), mc.unit_rows(rng, nb, dim)
    band_a, band_b = (np.arange(na) % 4).astype(np.float64), (np.arange(nb) % 4).astype(np.float64)
    band_a[3], band_b[9] = 100.0, 200.0
    band_a[7] = band_b[21] = 50.0
    A[12] = B[30]                                      # bands 0 and 2
    nz = A[12].astype(np.float64) + 0.05 * rng.standard_normal(dim) / np.sqrt(dim)
    B[32] = (nz / np.linalg.norm(nz)).astype(np.float32)                       # band 0
    v = mc.unit_rows(rng, 1, dim)[0]
    A[11] = v
    B[[5, 17, 40]] = v
    band_a[11] = band_b[5] = band_b[17] = band_b[40] = 1.0
    xy_a, xy_b = np.c_[np.zeros(na), band_a], np.c_[np.zeros(nb), band_b]
    xy_a[20] = np.nan
    xy_b[33, 1] = np.nan
    if kind == EPIPOLAR:
        M = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    else:
        M = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
        xy_a[24, 0], xy_a[25, 0] = 1.0, 2.0
    return dict(A=A, B=B, xy_a=xy_a, xy_b=xy_b, kind=kind, M=M, thr=0.01)


def check_edge_pair(case, run):
    """The planted rows of edge_pair under `run(case, **options) -> (matches0, scores0, n_matches)`."""
    adm = admissible(case["kind"], case["M"], case["thr"], case["xy_a"], case["xy_b"])
    assert not adm[3].any() and not adm[:, 9].any() and not adm[20].any() and not adm[:, 33].any()
    assert np.flatnonzero(adm[7]).tolist() == [21] and np.flatnonzero(adm[:, 21]).tolist() == [7]
    assert adm[11, [5, 17, 40]].all() and not adm[12, 30] and adm[12, 32]
    if case["kind"] == HOMOGRAPHY:
        assert not adm[24].any() and not adm[25].any()
    sim = mc.sim_chain(case["A"], case["B"])
    assert int(np.argmax(sim[12])) == 30
    ratio = run(case, **mc.CONFS["NN-ratio"])[0]
    mutual = run(case, **mc.CONFS["NN-mutual"])[0]
    assert ratio[7] == 21 and mutual[7] == 21
    assert mutual[12] == 32 and mutual[11] == 5
    for m in (ratio, mutual):
        assert m[3] == -1 and m[20] == -1 and 9 not in m and 33 not in m
        if case["kind"] == HOMOGRAPHY:
            assert m[24] == -1 and m[25] == -1


def gated_batch(dim=128, seed=29):
    """The images of matching_cases.batch_case (sizes 0, 1, 33, 129, 200) with keypoints in [-1, 1]^2 and eight pairs of mixed
    kind: (4, 4), (3, 4) epipolar, (3, 4) homography -- the same image pair under two models --, (4, 3), the empty image on either
    side, the one-descriptor image, and (3, 4) under a model of all NaN, which keeps no match.
    Returns (descs, xy, pairs, kinds, models, thrs)."""
    descs, _ = mc.batch_case(dim, seed)
    rng = np.random.default_rng(seed + 1)
    xy = [rng.uniform(-1, 1, (len(d), 2)) for d in descs]
    pairs = np.array([(4, 4), (3, 4), (3, 4), (4, 3), (0, 2), (2, 0), (1, 3), (3, 4)], dtype=np.int32)
    kinds = np.array([EPIPOLAR, EPIPOLAR, HOMOGRAPHY, HOMOGRAPHY, EPIPOLAR, HOMOGRAPHY, EPIPOLAR, EPIPOLAR], dtype=np.int32)
    models = np.stack([random_model(rng, k) for k in kinds])
    thrs = np.array([threshold_for(k, M, xy[a], xy[b], 0.3) for k, M, (a, b) in zip(kinds, models, pairs)])
    models[7] = np.nan
    return descs, xy, pairs, kinds, models, thrs


def twin_scene(seed=10, n_points=200, dim=64, desc_noise=0.03, kp_noise=0.5, focal=1000.0):
    """Repeated structure: two views of 2 n_points 3D points, point n_points + k carrying the descriptor of point k (its twin,
    somewhere else in space); per observation descriptor noise as in matching_cases.scene and keypoint noise in pixels;
    keypoints in shuffled order.  Two noisy copies of one descriptor can pass the ratio test against each other by chance (1 of
    400 rows at some seeds); the default seed is one at which the reference keeps no wrong match.  SIMPLE_PINHOLE cameras of focal
    length `focal`, principal point (500, 500).
    Returns dict(descriptors, keypoints, cameras (model id, params) per image name, pair, partner (per keypoint of image 1 the
    keypoint of image 2 of the same point), E (x2^t E x1 = 0 in the normalised plane, from the true poses))."""
    rng = np.random.default_rng(seed)
    n = 2 * n_points
    X = np.c_[rng.uniform(-1.2, 1.2, (n, 2)), rng.uniform(4.0, 8.0, n)]
    base = mc.unit_rows(rng, n_points, dim).astype(np.float64)
    base = np.concatenate([base, base])
    a = 0.1
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    t = np.array([-1.0, 0.1, 0.05])
    t /= np.linalg.norm(t)
    names = ("view1.jpg", "view2.jpg")
    desc, kps, order = {}, {}, {}
    for name, Xc in zip(names, (X, X @ R.T + t)):
        d = base + desc_noise * rng.standard_normal((n, dim)) / np.sqrt(dim)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        px = focal * Xc[:, :2] / Xc[:, 2:] + 500.0 + kp_noise * rng.standard_normal((n, 2))
        order[name] = rng.permutation(n)              # keypoint k shows point order[k]
        desc[name], kps[name] = d[order[name]].astype(np.float32), px[order[name]]
    where2 = np.empty(n, dtype=np.int64)
    where2[order[names[1]]] = np.arange(n)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    cams = {name: (0, np.array([focal, 500.0, 500.0])) for name in names}
    return dict(descriptors=desc, keypoints=kps, cameras=cams, pair=names, partner=where2[order[names[0]]], E=tx @ R, focal=focal)


def twin_normalised(scene):
    """The keypoints of twin_scene in the normalised plane of their SIMPLE_PINHOLE cameras (plain numpy)."""
    return {n: (scene["keypoints"][n] - scene["cameras"][n][1][1:3]) / scene["cameras"][n][1][0] for n in scene["pair"]}


def right_wrong(matches0, partner):
    """(right, wrong) of the kept matches of image 1 against the true partners."""
    kept = matches0 >= 0
    right = int((matches0[kept] == partner[kept]).sum())
    return right, int(kept.sum()) - right
