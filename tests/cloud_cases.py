"""The specification of pxr_cloud_nearest and pxr_cloud_voxel_fractions (include/pixsfm_hip.h) stated in numpy by brute force, and
the cases the CPU, lane-emulation and GPU tests share.  Expression orders are the header's: d2 = ((dx dx + dy dy) + dz dz) with
dx = q.x - r.x, the threshold one multiplication max_dist max_dist, the voxel floor(x / v) in float64, the fixed-point quotient
rint((w / n) 2^32) summed as int64.  numpy's float64 operations are single correctly rounded IEEE operations: nothing is fused."""
import numpy as np

INF = np.inf


def valid_rows(xyz):
    return np.isfinite(np.asarray(xyz, np.float64).reshape(-1, 3)).all(axis=1)


def dist2_matrix(query, ref):
    """d2 of every (query, reference) pair in the order of the specification."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = query[:, None, :] - ref[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(ref, query, max_dist, chunk_elems=1 << 21):
    """(index int32, dist2 float64) of pxr_cloud_nearest: the n_query x n_ref matrix in chunks of rows."""
    ref = np.ascontiguousarray(ref, np.float64).reshape(-1, 3)
    query = np.ascontiguousarray(query, np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        m2 = np.float64(max_dist) * np.float64(max_dist)
    nq, nr = len(query), len(ref)
    index, dist2 = np.full(nq, -1, np.int32), np.full(nq, INF)
    if nr == 0 or nq == 0:
        return index, dist2
    vr, vq = valid_rows(ref), valid_rows(query)
    rows = max(1, chunk_elems // nr)
    for i0 in range(0, nq, rows):
        q = query[i0:i0 + rows]
        d2 = dist2_matrix(q, ref)
        with np.errstate(invalid="ignore"):
            cand = vr[None, :] & vq[i0:i0 + rows, None] & (d2 <= m2)
        d2c = np.where(cand, d2, INF)
        best = np.argmin(d2c, axis=1)                                  # the first of equal minima: the lowest index
        low = d2c[np.arange(len(q)), best]
        best = np.where(np.isinf(low), np.argmax(cand, axis=1), best)  # (an infinite d2 can be a candidate when max_dist^2 overflows)
        has = cand.any(axis=1)
        index[i0:i0 + rows] = np.where(has, best, -1)
        dist2[i0:i0 + rows] = np.where(has, low, INF)
    return index, dist2


def voxel_fractions(xyz, dist2, voxel_size, tolerances):
    """(fractions float64 (n_tol,), n_voxels) of pxr_cloud_voxel_fractions, or None where it returns PXR_EINVAL for a voxel
    component of magnitude 2^20 or more."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    dist2 = np.ascontiguousarray(dist2, np.float64).reshape(-1)
    tol = np.asarray(tolerances, np.float64).reshape(-1)
    v = valid_rows(xyz)
    pts, d2 = xyz[v], dist2[v]
    if voxel_size == 0:
        inv, n_vox = np.arange(len(pts)), len(pts)
    else:
        with np.errstate(over="ignore"):
            c = np.floor(pts / np.float64(voxel_size))
        if not (np.abs(c) < 2.0 ** 20).all():
            return None
        _, inv = np.unique(c.astype(np.int64), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n_vox = int(inv.max()) + 1 if len(inv) else 0
    if n_vox == 0:
        return np.full(len(tol), np.nan), 0
    n_v = np.bincount(inv, minlength=n_vox).astype(np.float64)
    out = np.empty(len(tol))
    for k, t in enumerate(tol):
        with np.errstate(invalid="ignore"):
            within = d2 <= t * t
        w_v = np.bincount(inv[within], minlength=n_vox).astype(np.float64)
        q = np.rint((w_v / n_v) * 4294967296.0).astype(np.int64)
        out[k] = float(int(q.sum(dtype=np.int64))) * 2.0 ** -32 / float(n_vox)
    return out, n_vox


# ---- nearest-neighbour cases: name -> (ref, query, max_dist) ---------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 257)


def _near(rng, ref, n, spread):
    """n queries: reference points moved by up to `spread` per axis (or uniform in the unit cube when there is no reference)."""
    if len(ref) == 0:
        return rng.uniform(-1, 1, (n, 3))
    return ref[rng.integers(0, len(ref), n)] + rng.uniform(-spread, spread, (n, 3))


def size_case(n_ref, n_query):
    rng = np.random.default_rng(1000 * n_ref + n_query)
    ref = rng.uniform(-1, 1, (n_ref, 3))
    return ref, _near(rng, ref, n_query, 0.08), 0.1


def exact_pairs(s):
    """Pairs at exactly max_dist (offsets (3, 4, 0) s with max_dist 5 s, (2, 3, 6) s with 7 s) and the same pairs one ulp outside:
    case -> (ref, query, max_dist, inside) with `inside` the expected verdict per query (its reference is reference i)."""
    out = {}
    for off, m in (((3.0, 4.0, 0.0), 5.0), ((2.0, 3.0, 6.0), 7.0)):
        off, max_dist = np.array(off) * s, m * s
        base = np.array([[0.0, 0.0, 0.0], [-16.0, 8.0, 24.0], [12.0, -40.0, -8.0], [-3.0, -4.0, -28.0]]) * (8 * m * s)   # far apart
        query, ref, inside = [], [], []
        for sign in (1.0, -1.0):
            for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
                for b in base:
                    o = sign * off[list(perm)]
                    query.append(b)
                    ref.append(b + o)
                    inside.append(True)
                    k = int(np.argmax(np.abs(o)))                     # one ulp further out along the largest offset
                    far = b + 1024 * m * s                            # (integers times a power of two: every sum here is exact)
                    r = far + o
                    r[k] = np.nextafter(r[k], r[k] + np.sign(o[k]) * 1e300)
                    query.append(far)
                    ref.append(r)
                    inside.append(False)
        ref, query, inside = np.array(ref), np.array(query), np.array(inside)
        d2 = np.einsum("ii->i", dist2_matrix(query, ref))
        m2 = np.float64(max_dist) * np.float64(max_dist)
        assert (d2[inside] == m2).all() and (d2[~inside] > m2).all(), (off, s)   # exactly at max_dist in float64 / just outside
        out["exact_%g_%g" % (m, s)] = (ref, query, max_dist, inside)
    return out


EXACT_SCALES = (2.0 ** -10, 1.0, 2.0 ** 7)


def nearest_cases():
    cases = {}
    for nr in SIZES:
        for nq in SIZES:
            cases["size_%dx%d" % (nr, nq)] = size_case(nr, nq)
    rng = np.random.default_rng(77)
    ref = rng.uniform(-1, 1, (3000, 3))
    cases["random_3000x2000"] = (ref, _near(rng, ref, 2000, 0.06), 0.05)
    # every coordinate an exact multiple of max_dist, negatives included: points on cell faces, distances of exactly max_dist, ties
    m = 0.25
    cases["lattice"] = (m * rng.integers(-4, 5, (600, 3)), m * rng.integers(-5, 6, (500, 3)), m)
    m = 0.1                                                            # (not a binary fraction: the quotients round)
    cases["lattice_0.1"] = (m * rng.integers(-6, 7, (600, 3)).astype(np.float64), m * rng.integers(-7, 8, (500, 3)).astype(np.float64), m)
    for s in EXACT_SCALES:
        for name, (r, q, md, _) in exact_pairs(s).items():
            cases[name] = (r, q, md)
    # all references in one cell: one long bucket
    ref = rng.uniform(0.05, 0.95, (3000, 3))
    cases["one_cell"] = (ref, rng.uniform(-0.5, 1.5, (2000, 3)), 1.0)
    # many cells, far from the origin: the table's wrap-around
    ref = rng.uniform(-1e4, 1e4, (3000, 3))
    cases["spread"] = (ref, np.concatenate([_near(rng, ref, 1500, 0.008), rng.uniform(-1e4, 1e4, (500, 3))]), 0.01)
    # exact duplicates among the references: the lowest index wins
    ref = rng.uniform(-1, 1, (400, 3))
    ref[200:] = ref[rng.integers(0, 200, 200)]
    cases["duplicates"] = (ref, np.concatenate([ref[::3], _near(rng, ref, 300, 0.05)]), 0.1)
    # rows that are not valid in both clouds
    ref = rng.uniform(-1, 1, (300, 3))
    query = _near(rng, ref, 200, 0.05)
    ref[5, 0], ref[17, 2], ref[64, 1], ref[299, 0] = np.nan, INF, -INF, np.nan
    query[0, 1], query[63, 0], query[64, 2], query[199, 2] = np.nan, -INF, INF, np.nan
    query[10] = ref[6]
    cases["not_finite"] = (ref, query, 0.1)
    ref = rng.uniform(-1, 1, (500, 3))
    cases["identical"] = (ref, ref, 0.05)
    # max_dist^2 overflows: every valid pair is a candidate, an infinite d2 included
    ref = rng.uniform(-1, 1, (40, 3)) * 1e200
    cases["huge_max_dist"] = (ref, np.concatenate([_near(rng, ref, 30, 1e150), [[1e308, -1e308, 0.0]]]), 1e200)
    return {k: (np.ascontiguousarray(r, np.float64).reshape(-1, 3), np.ascontiguousarray(q, np.float64).reshape(-1, 3), float(md))
            for k, (r, q, md) in cases.items()}


def many_chunks_case():
    """(ref, query, max_dist) with 2^19 + 12 reference points: a table of 2^21 buckets, which the scan cuts into 512 chunks of 4096
    -- more chunks than the workgroup that scans their totals has threads, so a thread owns two.  Not in NEAREST_CASES: the
    lane emulation would spend minutes on it; 64 queries keep the brute force at the size of the other cases."""
    rng = np.random.default_rng(19)
    ref = rng.uniform(-1, 1, (2 ** 19 + 12, 3))
    return ref, _near(rng, ref, 64, 0.008), 0.01


# ---- voxel cases: name -> (xyz, dist2, voxel_size, tolerances) -------------------------------------------------------------------
TOL3 = (0.01, 0.02, 0.05)
TOL8 = (0.005, 0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.5)


def voxel_cases():
    rng = np.random.default_rng(5)
    cases = {}

    def d2_of(n):
        d = rng.uniform(0, 0.06, n) ** 2
        d[rng.random(n) < 0.2] = INF                                   # queries without a candidate
        return d
    # points on voxel faces, negative coordinates: floor is not a truncation
    xyz = 0.25 * rng.integers(-9, 10, (700, 3)) * rng.choice([1.0, 0.5], (700, 3))
    cases["faces"] = (xyz, d2_of(700), 0.25, TOL3)
    cases["faces_0.01"] = (0.01 * rng.integers(-30, 31, (700, 3)).astype(np.float64), d2_of(700), 0.01, TOL3)
    cases["one_voxel"] = (rng.uniform(0.0, 0.999, (1000, 3)) - 3.0, d2_of(1000), 1.0, TOL3)
    grid = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5
    cases["own_voxel"] = (grid, d2_of(len(grid)), 1.0, TOL3)
    xyz = rng.normal(0, 0.3, (5000, 3))
    cases["zero_size"] = (xyz, d2_of(5000), 0.0, TOL3)
    cases["random_5000"] = (xyz, d2_of(5000), 0.1, TOL3)
    cases["eight_tolerances"] = (xyz[:777], rng.uniform(0, 0.6, 777) ** 2, 0.1, TOL8)
    bad = xyz[:300].copy()
    bad[3, 1], bad[64, 0], bad[299, 2] = np.nan, INF, -INF
    cases["not_finite"] = (bad, d2_of(300), 0.05, TOL3)
    cases["no_valid_point"] = (np.full((5, 3), np.nan), np.zeros(5), 0.05, TOL3)
    cases["empty"] = (np.zeros((0, 3)), np.zeros(0), 0.05, TOL3)
    cases["all_within"] = (xyz[:100], np.zeros(100), 0.05, TOL3)
    # a component of 2^20 voxels or more (positive: exactly 2^20; negative: -2^20 is refused too, -2^20 + 1 is not)
    far = xyz[:50].copy()
    far[7, 2] = 2.0 ** 20 * 0.5
    cases["out_of_range"] = (far, d2_of(50), 0.5, TOL3)
    far = xyz[:50].copy()
    far[49, 0] = -(2.0 ** 20) * 0.5
    cases["out_of_range_negative"] = (far, d2_of(50), 0.5, TOL3)
    edge = xyz[:50].copy()
    edge[0] = [-(2.0 ** 20 - 1) * 0.5, (2.0 ** 20 - 0.5) * 0.5, 0.0]
    cases["range_edge"] = (edge, d2_of(50), 0.5, TOL3)
    return {k: (np.ascontiguousarray(x, np.float64).reshape(-1, 3), np.ascontiguousarray(d, np.float64), float(v), tuple(t))
            for k, (x, d, v, t) in cases.items()}


_REFERENCE = {}


def nearest_reference(name):
    """The brute-force result of a case, computed once per process."""
    key = ("nearest", name)
    if key not in _REFERENCE:
        ref, query, max_dist = NEAREST_CASES[name]
        _REFERENCE[key] = nearest(ref, query, max_dist)
    return _REFERENCE[key]


def voxel_reference(name):
    key = ("voxel", name)
    if key not in _REFERENCE:
        _REFERENCE[key] = voxel_fractions(*VOXEL_CASES[name])
    return _REFERENCE[key]


NEAREST_CASES = nearest_cases()
VOXEL_CASES = voxel_cases()
