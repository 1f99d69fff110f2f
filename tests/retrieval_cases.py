"""The retrieval stage's reference, written from the specification (include/pixsfm_hip.h) and not from the
kernels: the float32 fmaf chain of matching_cases.sim_chain, the selections stated with argmax / lexsort (the kernels scan and
merge), the fixed-point sums in int64 with np.add.at (the kernels use integer atomics), the ordered float64 sums with np.cumsum,
numpy's correctly rounded float64 sqrt and division -- and the generators of the test cases, all with fixed seeds."""
import numpy as np

from matching_cases import sim_chain, unit_rows

F32 = np.float32


# ---- rules 1-3 ----------------------------------------------------------------------------------------------------------------------
def valid_rows(X):
    X = np.asarray(X, F32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(X) & (np.abs(X) <= 1)).all(axis=1)


def assign(X, C):
    """assign[i] = the c of the largest sim(x_i, C_c), ties to the lowest c; -1 for an invalid row or when every sim is NaN."""
    X, C = np.asarray(X, F32), np.asarray(C, F32)
    if len(X) == 0:
        return np.empty(0, np.int32)
    sim = sim_chain(X, C)
    nan = np.isnan(sim)
    best = np.argmax(np.where(nan, F32(-np.inf), sim), axis=1)
    return np.where(valid_rows(X) & ~nan.all(axis=1), best, -1).astype(np.int32)


def quantise(X):
    return np.rint(np.asarray(X, F32).astype(np.float64) * 2.0 ** 32).astype(np.int64)


def sums(X, a, K):
    """S (K, D) int64 and cnt (K,) of the rows of X with assignment a >= 0."""
    X = np.asarray(X, F32)
    S, keep = np.zeros((K, X.shape[1]), np.int64), a >= 0
    np.add.at(S, a[keep], quantise(X[keep]))
    return S, np.bincount(a[keep], minlength=K).astype(np.int32)


def _ordered_sum_of_squares(v):
    """sum_k v[..., k]^2 in float64 in ascending k."""
    return np.cumsum(v * v, axis=-1)[..., -1]


# ---- rule 4 -------------------------------------------------------------------------------------------------------------------------
def training_rows(n_total, max_train):
    n_train = min(n_total, max_train)
    return np.array([j * n_total // n_train for j in range(n_train)], dtype=np.int64)


def vocab_train(X, K, n_iterations, max_train=262144):
    """(centroids (K, D) float32, cnt (K,) int32, n_empty)."""
    X = np.asarray(X, F32)
    T = X[training_rows(len(X), max_train)]
    n_train = len(T)
    assert K <= n_train
    C = T[[c * n_train // K for c in range(K)]].copy()
    cnt = np.zeros(K, np.int32)
    for _ in range(n_iterations):
        S, cnt = sums(T, assign(T, C), K)
        s = S.astype(np.float64)
        n2 = _ordered_sum_of_squares(s)
        for c in range(K):
            if cnt[c] > 0 and n2[c] > 0:
                C[c] = (s[c] / np.sqrt(n2[c])).astype(F32)
    return C, cnt, int((cnt == 0).sum())


# ---- rule 5 -------------------------------------------------------------------------------------------------------------------------
def vlad(descs, C):
    """(G (n_images, K D) float32, assign (n_total,) int32, counts (n_images, K) int32) of a list of (n, D) arrays."""
    C = np.asarray(C, F32)
    K, D = C.shape
    G, A, N = np.zeros((len(descs), K * D), F32), [], np.zeros((len(descs), K), np.int32)
    for m, X in enumerate(descs):
        X = np.asarray(X, F32).reshape(-1, D)
        a = assign(X, C)
        S, cnt = sums(X, a, K)
        v = S.astype(np.float64) * 2.0 ** -32 - cnt.astype(np.float64)[:, None] * C.astype(np.float64)
        b2 = np.where(cnt > 0, _ordered_sum_of_squares(v), 0.0)
        nne = int((b2 > 0).sum())
        for c in range(K):
            if b2[c] > 0:
                G[m, c * D:(c + 1) * D] = (v[c] / (np.sqrt(b2[c]) * np.sqrt(np.float64(nne)))).astype(F32)
        A.append(a)
        N[m] = cnt
    return G, (np.concatenate(A) if A else np.empty(0, np.int32)), N


# ---- rule 6 -------------------------------------------------------------------------------------------------------------------------
def topk(Q, DB, num_matched, query_self=None, mask=None, min_score=None):
    """(top_index (n_query, num_matched) int32 padded with -1, top_sim float32 padded with 0, n_found (n_query,) int32)."""
    Q, DB = np.asarray(Q, F32), np.asarray(DB, F32)
    nq, ndb = len(Q), len(DB)
    sim = sim_chain(Q, DB) if nq and ndb else np.zeros((nq, ndb), F32)
    top, val, found = np.full((nq, num_matched), -1, np.int32), np.zeros((nq, num_matched), F32), np.zeros(nq, np.int32)
    for i in range(nq):
        cand = ~np.isnan(sim[i])
        if mask is not None:
            cand &= np.asarray(mask).reshape(nq, ndb)[i] != 0
        if query_self is not None and query_self[i] >= 0:
            cand[query_self[i]] = False
        if min_score is not None and np.isfinite(min_score):
            with np.errstate(invalid="ignore"):
                cand &= sim[i] >= F32(min_score)
        j = np.flatnonzero(cand)
        j = j[np.lexsort((j, -sim[i, j].astype(np.float64)))][:num_matched]       # by sim descending, then j ascending
        top[i, :len(j)], val[i, :len(j)], found[i] = j, sim[i, j], len(j)
    return top, val, found


def pairs_from_retrieval(global_descriptors, num_matched, query_names=None, db_names=None, min_score=None, match_mask=None):
    """The list api.retrieval.pairs_from_retrieval returns, from this reference."""
    names = list(global_descriptors)
    query_names = names if query_names is None else list(query_names)
    db_names = names if db_names is None else list(db_names)
    Q = np.stack([global_descriptors[n] for n in query_names])
    DB = np.stack([global_descriptors[n] for n in db_names])
    self_ = np.array([db_names.index(n) if n in db_names else -1 for n in query_names], np.int32)
    top, _, found = topk(Q, DB, num_matched, self_, match_mask, min_score)
    return [(q, db_names[j]) for i, q in enumerate(query_names) for j in top[i, :found[i]]]


# ---- generators ---------------------------------------------------------------------------------------------------------------------
ASSIGN_SHAPES = [(1, 1, 4), (37, 2, 128), (33, 31, 128), (129, 64, 128), (300, 256, 128), (70, 5, 130), (40, 33, 512)]


def assignment_case(n, K, D, seed):
    """Unit rows and unit centroids, and as far as n and K allow: two bit-identical centroids (0 and K - 1) with a row equal to
    them (the lowest index must win), a row with a NaN, a row with an entry of 1.5, a row equal to another centroid."""
    rng = np.random.default_rng(seed)
    X, C = unit_rows(rng, n, D), unit_rows(rng, K, D)
    if K >= 2:
        C[K - 1] = C[0]
    X[0] = C[0]
    if n >= 4:
        X[1, D // 2] = np.nan
        X[2, D - 1] = 1.5
        X[3] = C[K // 2]
    return X, C


def clustered_rows(rng, n, centres, noise=0.25):
    """n unit rows around randomly chosen rows of `centres`."""
    c = centres[rng.integers(0, len(centres), n)].astype(np.float64)
    x = c + noise * rng.standard_normal(c.shape) / np.sqrt(c.shape[1])
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


AGG_SIZES = [0, 1, 63, 64, 65, 257, 1025]


def aggregation_case(K, D, seed):
    """Centroids and a batch of images: the sizes of AGG_SIZES, an image whose rows all go to one centroid (noisy copies of it),
    an image with a single row equal to its centroid (a zero block), an image of invalid rows only."""
    rng = np.random.default_rng(seed)
    C = unit_rows(rng, K, D)
    C[K // 2] = np.round(C[K // 2] * 2.0 ** 20) / 2.0 ** 20      # multiples of 2^-20: q() is exact on them, the residual of a copy is 0
    descs = [clustered_rows(rng, n, C) if n else np.empty((0, D), F32) for n in AGG_SIZES]
    descs.append(clustered_rows(rng, 40, C[K - 1:K], noise=0.05))
    descs.append(C[K // 2:K // 2 + 1].copy())
    bad = unit_rows(rng, 5, D)
    bad[:, 0] = [np.nan, np.inf, -np.inf, 1.5, -1.25]
    descs.append(bad)
    descs[4][7, D - 1] = np.nan                        # and an invalid row inside an ordinary image
    return descs, C


TRAIN_CASES = {         # name: (n_total, K, D, iterations, max_train)
    "300x4x8": (300, 4, 8, 3, 262144),
    "1000x64x128": (1000, 64, 128, 2, 262144),
    "max_train_below_n": (700, 8, 24, 3, 256),
    "duplicates": (200, 6, 16, 1, 262144),     # one iteration: the later duplicate cannot win a row, whatever the data
    "K_equals_n_train": (90, 32, 12, 2, 32),
}


def training_case(name):
    n, K, D, iters, max_train = TRAIN_CASES[name]
    rng = np.random.default_rng(500 + sorted(TRAIN_CASES).index(name))
    X = clustered_rows(rng, n, unit_rows(rng, max(K // 2, 2), D), noise=0.5)
    if name == "duplicates":                           # initial rows floor(c n / K) for c = 2 and 4 are bit-identical
        X[4 * n // K] = X[2 * n // K]
    return X, K, iters, max_train


TOPK_SHAPES = [(1, 1, 8, 1), (5, 5, 130, 2), (12, 40, 8192, 5), (3, 300, 32768, 20)]


def global_rows(rng, n, dim):
    return unit_rows(rng, n, dim)


def ring_scene(n_images=24, n_points=600, window=5, dim=32, noise=0.15, n_extra=10, seed=77):
    """A ring of images; point p sits at angle 2 pi p / n_points and is seen by the `window` images nearest to it.  A random unit
    descriptor per point, perturbed per observation and renormalised; n_extra unmatched descriptors per image; shuffled.
    Returns (descriptors {name: (n, dim) float32}, points {name: set of point ids})."""
    rng = np.random.default_rng(seed)
    base = unit_rows(rng, n_points, dim).astype(np.float64)
    desc, pts = {}, {}
    for m in range(n_images):
        centre = (m + 0.5) * n_points / n_images
        d = np.abs((np.arange(n_points) - centre + n_points / 2) % n_points - n_points / 2)
        seen = np.flatnonzero(d < window * n_points / n_images / 2)
        x = base[seen] + noise * rng.standard_normal((len(seen), dim)) / np.sqrt(dim)
        x = np.concatenate([x / np.linalg.norm(x, axis=1, keepdims=True), unit_rows(rng, n_extra, dim)])
        name = "ring%02d.jpg" % m
        desc[name], pts[name] = x[rng.permutation(len(x))].astype(F32), set(seen.tolist())
    return desc, pts


def connected(names, pairs):
    parent = {n: n for n in names}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        parent[find(a)] = find(b)
    return len({find(n) for n in names}) == 1


PIPELINE_PARAMS = [1200.0, 500.0, 500.0, 0.02]                         # SIMPLE_RADIAL, 1000 x 1000


def pipeline_scene(n_images=12, n_points=300, views=5, n_extra=20, dim=32, sigma=0.3, desc_noise=0.15, seed=5):
    """A ring of cameras around points in a cube; every point is seen by `views` neighbouring images.  Keypoints (noisy
    projections) with descriptors (a unit vector per point, perturbed per observation), plus keypoints that nothing else sees.
    Returns (names, keypoints {name: (n, 2)}, descriptors {name: (n, dim) float32})."""
    from pixsfm_amd import synthetic
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    X = rng.uniform(-1, 1, (n_points, 3))
    base = unit_rows(rng, n_points, dim).astype(np.float64)
    kps, descs = {n: [] for n in names}, {n: [] for n in names}
    for p in range(n_points):
        first = rng.integers(n_images)
        for j in range(views):
            i = (first + j) % n_images
            kps[names[i]].append(synthetic.project(2, PIPELINE_PARAMS, qvec[i], tvec[i], X[p]) + rng.normal(0, sigma, 2))
            d = base[p] + desc_noise * rng.standard_normal(dim) / np.sqrt(dim)
            descs[names[i]].append(d / np.linalg.norm(d))
    for n in names:
        kps[n] += list(rng.uniform(0, 1000, (n_extra, 2)))
        descs[n] += list(unit_rows(rng, n_extra, dim))
        order = rng.permutation(len(kps[n]))
        kps[n], descs[n] = np.array(kps[n])[order], np.array(descs[n], dtype=F32)[order]
    return names, kps, descs
