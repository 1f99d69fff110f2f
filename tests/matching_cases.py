"""The descriptor matcher's reference, written from the specification (include/pixsfm_hip.h) and not from
the kernels: the float32 fmaf chain through a C helper (tests/host/sim_fmaf.c), the selection rules in numpy float32 stated with
argmax / masking (the kernels scan and merge), and the generators of the test cases, all with fixed seeds."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFS = {          # hloc's names
    "NN-mutual": dict(ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True),
    "NN-ratio": dict(ratio_threshold=0.8, distance_threshold=0.0, do_mutual_check=True),
    "NN-superpoint": dict(ratio_threshold=0.0, distance_threshold=0.7, do_mutual_check=True),
}
# every shape runs with these four
OPTION_SETS = dict(CONFS, **{"NN-ratio-one-way": dict(ratio_threshold=0.8, distance_threshold=0.0, do_mutual_check=False)})

_helper = None
_helper_dir = None


def build_sim_helper(directory):
    """gcc -O1 -ffp-contract=off tests/host/sim_fmaf.c -> a shared object in `directory`; returns the loaded library."""
    out = os.path.join(str(directory), "libsim_fmaf.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                           os.path.join(HERE, "host", "sim_fmaf.c"), "-o", out, "-lm"])
    lib = ctypes.CDLL(out)
    lib.sim_fmaf.restype = None
    lib.sim_fmaf.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    return lib


def sim_helper():
    global _helper, _helper_dir
    if _helper is None:
        _helper_dir = tempfile.TemporaryDirectory(prefix="sim_fmaf_")
        _helper = build_sim_helper(_helper_dir.name)
    return _helper


def sim_chain(A, B):
    """sim[i][j] = the float32 value of s = 0; for k ascending: s = fmaf(A[i][k], B[j][k], s)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[1]
    sim = np.empty((A.shape[0], B.shape[0]), dtype=np.float32)
    if sim.size:
        sim_helper().sim_fmaf(A.ctypes.data, B.ctypes.data, A.shape[0], B.shape[0], A.shape[1], sim.ctypes.data)
    return sim


def _select(sim, ratio_threshold, distance_threshold, skip_ratio):
    """Forward selection over the rows of `sim` (float32): m (n,) int32."""
    f = np.float32
    n, m = sim.shape
    if m == 0:
        return np.full(n, -1, np.int32), np.full(n, -np.inf, f)
    s = np.where(np.isnan(sim), f(-np.inf), sim).astype(f)           # a NaN never wins
    best = np.argmax(s, axis=1)                                       # the first of the largest: the lowest index
    rows = np.arange(n)
    s1 = s[rows, best]
    rest = s.copy()
    rest[rows, best] = -np.inf
    s2 = rest.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        d1 = f(2) * (f(1) - s1)
        d2 = f(2) * (f(1) - s2)
        ok = s1 > -np.inf
        if ratio_threshold > 0 and not skip_ratio:
            ok &= d1 <= f(ratio_threshold * ratio_threshold) * d2
        if distance_threshold > 0:
            ok &= d1 <= f(distance_threshold * distance_threshold)
    return np.where(ok, best, -1).astype(np.int32), s1.astype(f)


def match_from_sim(sim, ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True):
    """(matches0 int32 (na,), scores0 float32 (na,), n_matches) of one pair from its similarity matrix."""
    sim = np.asarray(sim, dtype=np.float32)
    na, nb = sim.shape
    skip = na == 1 or nb == 1
    m0, s1 = _select(sim, ratio_threshold, distance_threshold, skip)
    if do_mutual_check:
        m1, _ = _select(np.ascontiguousarray(sim.T), ratio_threshold, distance_threshold, skip)
        keep = m0 >= 0
        keep[keep] = m1[m0[keep]] == np.flatnonzero(keep)
        m0 = np.where(keep, m0, -1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        scores = np.where(m0 >= 0, (s1 + np.float32(1)) / np.float32(2), np.float32(0)).astype(np.float32)
    return m0, scores, int((m0 >= 0).sum())


def match_reference(A, B, options=None):
    return match_from_sim(sim_chain(A, B), **(options or CONFS["NN-mutual"]))


def reference_batch(descriptors, pairs, options=None):
    """The flat outputs of pxr_match_descriptors: matches0, scores0, n_matches, pair_offsets."""
    res = [match_reference(descriptors[a], descriptors[b], options) for a, b in pairs]
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in res])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.empty(0, dt)   # noqa: E731
    return cat(0, np.int32), cat(1, np.float32), np.array([r[2] for r in res], dtype=np.int32), off


# ---- generators -------------------------------------------------------------------------------------------------------------------
def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    return x.astype(np.float32)


def pair_case(na, nb, dim, seed, shared=0.6, noise=0.05):
    """Two images: `shared` of the smaller one are noisy copies of descriptors of the other (at shuffled places), the rest random
    unit vectors -- so that every conf keeps some matches and drops some."""
    rng = np.random.default_rng(seed)
    A, B = unit_rows(rng, na, dim), unit_rows(rng, nb, dim)
    k = int(shared * min(na, nb))
    ia, ib = rng.permutation(na)[:k], rng.permutation(nb)[:k]
    nz = B[ib].astype(np.float64) + noise * rng.standard_normal((k, dim)) / np.sqrt(dim)
    A[ia] = (nz / np.linalg.norm(nz, axis=1, keepdims=True)).astype(np.float32)
    return A, B


GPU_SHAPES = [(1, 1, 4), (1, 37, 128), (37, 1, 128), (32, 32, 2), (33, 31, 128), (129, 65, 128), (300, 200, 256), (70, 90, 5),
              (70, 90, 130), (40, 40, 512)]


def tie_case(copies_in_b=True, dim=128, seed=3):
    """One side holds three bit-identical copies of a descriptor at 5, 17, 40; the other side holds it too (at 11)."""
    rng = np.random.default_rng(seed)
    A, B = unit_rows(rng, 50, dim), unit_rows(rng, 64, dim)
    v = unit_rows(rng, 1, dim)[0]
    A[11] = v
    B[[5, 17, 40]] = v
    return (A, B) if copies_in_b else (B, A)


def scene(n_images=5, n_points=60, n_extra=12, dim=64, p_seen=0.7, noise=0.03, seed=11):
    """A synthetic set of images whose keypoints carry descriptors: a random unit vector per 3D point plus per-observation noise,
    renormalised; n_extra unmatched keypoints per image; keypoints in shuffled order.
    Returns (descriptors {name: (n, dim) float32}, point_of_keypoint {name: (n,) point id or -1}, pairs [(name1, name2)])."""
    rng = np.random.default_rng(seed)
    base = unit_rows(rng, n_points, dim).astype(np.float64)
    desc, owner = {}, {}
    for m in range(n_images):
        seen = np.flatnonzero(rng.random(n_points) < p_seen)
        d = base[seen] + noise * rng.standard_normal((len(seen), dim)) / np.sqrt(dim)
        d = np.concatenate([d, unit_rows(rng, n_extra, dim)])
        ids = np.concatenate([seen, np.full(n_extra, -1)])
        order = rng.permutation(len(ids))
        d = d[order] / np.linalg.norm(d[order], axis=1, keepdims=True)
        name = "image%02d.jpg" % m
        desc[name], owner[name] = d.astype(np.float32), ids[order].astype(np.int64)
    names = list(desc)
    pairs = [(names[i], names[j]) for i in range(n_images) for j in range(i + 1, n_images)]
    return desc, owner, pairs


def batch_case(dim=128, seed=29):
    """Five images of sizes 0, 1, 33, 129, 200 and six pairs: (i, i), (a, b), (b, a), the empty image on either side, and the
    one-descriptor image."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 33, 129, 200]
    descs = [unit_rows(rng, n, dim) for n in sizes]
    # images 3 and 4 share descriptors, so that (3, 4) / (4, 3) have mutual matches worth comparing
    k = 80
    ia, ib = rng.permutation(129)[:k], rng.permutation(200)[:k]
    nz = descs[4][ib].astype(np.float64) + 0.05 * rng.standard_normal((k, dim)) / np.sqrt(dim)
    descs[3][ia] = (nz / np.linalg.norm(nz, axis=1, keepdims=True)).astype(np.float32)
    descs[1][0] = descs[2][7]
    pairs = np.array([(4, 4), (3, 4), (4, 3), (0, 2), (2, 0), (1, 3)], dtype=np.int32)
    return descs, pairs
