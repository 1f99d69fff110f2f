"""Scenes of the iterative Schur solver's tests, shared by the CPU file (tests/test_oracle_pcg.py: the oracle's own step and the
condition of every scene as a reference) and the GPU file (tests/test_ba_pcg_precond_gpu.py).

DECOUPLED: scenes whose reduced camera system S is block diagonal over exactly the preconditioner's blocks (geom_cases.
make_decoupled_case: images 0-2 fully constant, every point seen by them and by ONE variable image; one camera per image).
INEXACT: the ramp-form scenes on which the GPU's inexact trajectory is compared with the oracle's."""
import functools

import numpy as np

import geom_cases

PINHOLE, FULL_OPENCV = 1, 6
NUM_PARAMS = {PINHOLE: 4, FULL_OPENCV: 12}
CAUCHY = geom_cases.RAMP_LOSS


def _all_but(*free):
    return 0xFFF & ~sum(1 << a for a in free)


# name: models (one id or one per camera), variable images, cam_const_mask per model, block rows per image, DC, lane-group width G
#                                                                     FULL_OPENCV: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
_MIXED = [FULL_OPENCV, PINHOLE, FULL_OPENCV] + [FULL_OPENCV, PINHOLE] * 3
DECOUPLED = {
    "pinhole8": dict(models=PINHOLE, nv=5, seed=11, cmask={PINHOLE: 0b1100}, rows=[0] * 3 + [8] * 5, DC=8, G=8),
    "opencv12": dict(models=FULL_OPENCV, nv=5, seed=12, cmask={FULL_OPENCV: _all_but(0, 1, 4, 5, 6, 7)}, rows=[0] * 3 + [12] * 5, DC=12, G=16),
    "opencv18": dict(models=FULL_OPENCV, nv=5, seed=13, cmask={FULL_OPENCV: 0}, rows=[0] * 3 + [18] * 5, DC=18, G=32),
    # images 3 .. 8: FULL_OPENCV, PINHOLE alternating; image 5 keeps t_x and t_z (a pose part of 4 rows), image 7 is pose-constant
    # with free intrinsics (a block of the 12 intrinsics alone)
    "mixed": dict(models=_MIXED, nv=6, seed=14, cmask={PINHOLE: 0b1100, FULL_OPENCV: 0}, rows=[0] * 3 + [18, 8, 16, 8, 12, 8], DC=18, G=32),
}
POINTS_PER_IMAGE = 30


def lane_group(DC):
    """launch_by_g of csrc/pxr_ba_pcg.hip"""
    return 8 if DC <= 8 else (16 if DC <= 16 else 32)


@functools.lru_cache(maxsize=None)
def decoupled(name, ramp=False):
    """(problem, gauge) of a DECOUPLED scene"""
    spec = DECOUPLED[name]
    prob = geom_cases.make_decoupled_case(spec["models"], spec["nv"], POINTS_PER_IMAGE, seed=spec["seed"], ramp=ramp)
    n_img, n_pt = len(prob["image_camera"]), len(prob["xyz"])
    assert list(prob["image_camera"]) == list(range(n_img))                  # one camera per image
    pose_const = np.zeros(n_img, np.uint8); pose_const[:3] = 1
    tmask = np.zeros(n_img, np.uint8)
    cmask = np.array([spec["cmask"][int(m)] for m in prob["cam_model"]], np.uint16)
    for c in range(3):
        cmask[c] = (1 << NUM_PARAMS[int(prob["cam_model"][c])]) - 1          # every parameter bit: the camera is constant
    if name == "mixed":
        tmask[5] = 0b101
        pose_const[7] = 1
    # the premise: no point is seen by two variable images
    var_img = {i for i in range(n_img) if spec["rows"][i] > 0}
    seen = {}
    for im, pt in zip(prob["obs_image"], prob["obs_point"]):
        if int(im) in var_img:
            seen.setdefault(int(pt), set()).add(int(im))
    assert len(seen) == n_pt and all(len(v) == 1 for v in seen.values())
    return prob, (pose_const, tmask, cmask, np.zeros(n_pt, np.uint8))


# name: how the scene is made.  `wide`: the scene of that id of tests/test_ba_wide_blocks_gpu.py (FULL_OPENCV, everything free:
# g = 18-row joint blocks, i = one camera shared by all images: a 12-row intrinsics block with an entry from every image).
INEXACT = {
    "six": dict(make_case=dict(n_cams=6, n_points=60, obs_per_point=4, seed=0)),
    "six_shared": dict(make_case=dict(n_cams=6, n_points=60, obs_per_point=4, seed=0, shared_camera=True)),
    "g": dict(wide="g"),
    "i": dict(wide="i"),
}
INEXACT_ITERATIONS = 7
# relative_decrease and trust_region_radius per iteration, GPU against the oracle: ten times the largest difference between the oracle's
# unperturbed and 1e-13-perturbed runs (7.0e-9: tests/test_ba_pcg_precond_gpu.py), rounded up to a power of ten; the ceiling is 1e-6
PER_ITERATION_RTOL = 1e-7
LINEAR_CAPS = (200, 3)             # max_linear_solver_iterations: the default (the Q test ends the solves) and a cap that ends most


@functools.lru_cache(maxsize=None)
def inexact(name):
    """(ramp-form problem, gauge) of an INEXACT scene"""
    spec = INEXACT[name]
    if "wide" in spec:
        import test_ba_wide_blocks_gpu as wide
        return wide.scene(spec["wide"])
    from test_ba_solve_gpu import _gauge
    prob = geom_cases.make_case(**spec["make_case"])
    return prob, _gauge(prob)


def perturbed(prob, rel=1e-13, seed=99):
    """the problem with every pose, intrinsic and point coordinate moved by `rel` relative"""
    rng = np.random.default_rng(seed)
    out = dict(prob)
    for key in ("qvec", "tvec", "cam_params", "xyz"):
        a = np.asarray(prob[key], dtype=np.float64)
        out[key] = a * (1.0 + rel * rng.uniform(-1.0, 1.0, a.shape))
    return out


def oracle_iterative(prob, gauge, max_iterations, cap=200, eta=0.1, r_tolerance=-1.0):
    """(summary, trace, (q, t, k, X)) of the oracle's LM loop with the iterative reduced step on a ramp-form problem"""
    import pxo
    s, tr, q, t, k, X = pxo.ba_solve_iterative(prob, pxo.cfg(l2_normalize=False), pxo.loss(*CAUCHY), *gauge,
                                               pxo.lm_options(max_iterations=max_iterations), pxo.linear_options(cap, eta, r_tolerance))
    geom_cases.assert_inside(prob, q, t, k, X, what="the oracle's iterative solution")
    return s, tr, (q, t, k, X)


@functools.lru_cache(maxsize=None)
def inexact_oracle(name, cap):
    """the oracle's inexact solve of an INEXACT scene: computed once, shared, left unchanged"""
    prob, gauge = inexact(name)
    return oracle_iterative(prob, gauge, INEXACT_ITERATIONS, cap)


def decisions(trace):
    return [(e["cg_iterations"], e["cg_stop"], e["step_is_valid"], e["step_is_successful"]) for e in trace]


def relative_gap(pa, pb):
    return max(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()) for a, b in zip(pa, pb))
