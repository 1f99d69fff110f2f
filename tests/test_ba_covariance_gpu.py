"""GPU: covariance of a bundle adjustment (pxr_ba_covariance, engine._BABase.covariance) against the inverse of the oracle's
Gauss-Newton matrix.

Reference.  The oracle's Jacobian of every residual block (geom_cases.oracle_eval(..., want_J=True): columns q(4) t(3) X(3) k(12)),
corrected as Ceres' Corrector does (corrector.cc: J~ = sqrt(rho') (J - alpha / s r r^T J), the second-order term only where
rho'' > 0), the quaternion columns taken to the tangent with QuaternionManifold::PlusJacobian, the variable columns in the order
of column_of (csrc/pxr_ba_structure.h) followed by three per variable point.  H = J~^T J~ in long double, its Cholesky factor L
and Sigma_ref = inv(L)^T inv(L) in long double (tests/spd_inverse_cases.py); every pose, intrinsics and point block and the dense
camera part are taken from Sigma_ref.

Comparison, whitened.  For a block with index set I, Delta = Sigma_gpu[I, I] - Sigma_ref[I, I] placed in a zero matrix, the
quantity is e = max |L^T Delta L|: to first order L^T (inv(H + dH) - inv(H)) L = -inv(L) dH inv(L)^T, a RELATIVE error of H that
does not grow with its conditioning.  Bound: 64 x the same quantity of numpy's float64 inverse of the float64 H (the margin
covers another order of summation and the scaling), plus the term of the solver's fixed-point accumulators:
  every addend of U and of the Schur complement is rounded to a grid of step q = 2^(ceil(log2(max(1, 4 sqrt(cost)))) - 62) on the
  SCALED system (det_scale_for, md = 1/8: the scaled diagonal is below 1), an entry takes at most n_obs addends from k_img and
  n_obs from the Schur kernel, each off by at most q / 2:  |dS_s| <= n_obs q elementwise, ||dS_s||_2 <= n_c n_obs q.  With
  H_s = D H D the scaled matrix (D the columns' powers of two, 1 on the points) and L_s its factor,
  max |inv(L_s) dH_s inv(L_s)^T| <= ||dS_s||_2 / lambda_min(H_s); the powers of two are taken from the reference's diagonal here,
  the device's may differ by one step per column (a factor 4 in lambda_min):
      quantum term = 4 n_c n_obs q / lambda_min(H_s).
Independently, every compared block agrees with the reference to 1e-6 relative in Frobenius norm.

Measured on an MI355X (case: whitened error e, numpy's, quantum term): see the table printed by each test (-s) and DESIGN 27.
"""
import functools
import os

import numpy as np
import pytest

import chol_cases as cc
import geom_cases
import spd_inverse_cases as sic

pytestmark = pytest.mark.gpu

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_geom_solve_bits.npz")
TRIVIAL, CAUCHY = ("trivial", 1.0), ("cauchy", 1.0)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def _gauge(prob, cam_const=None):
    """two constant poses; intrinsics: the principal point constant, focal length and distortion variable (cam_const: a mask for
    every camera instead)"""
    from pixsfm_amd._lib import CAMERA_NUM_PARAMS
    n_img, n_cam, n_pt = len(prob["image_camera"]), len(prob["cam_model"]), len(prob["xyz"])
    pose_const = np.zeros(n_img, np.uint8)
    pose_const[:2] = 1
    cmask = np.zeros(n_cam, np.uint16)
    for c, m in enumerate(prob["cam_model"]):
        pp = (2, 3) if int(m) in (1, 4, 5, 6, 7, 10) else (1, 2)
        cmask[c] = sum(1 << a for a in pp) if cam_const is None else cam_const & ((1 << CAMERA_NUM_PARAMS[int(m)]) - 1)
    return [pose_const, np.zeros(n_img, np.uint8), cmask, np.zeros(n_pt, np.uint8)]


def _with_outliers(prob):
    """every ninth keypoint moved by 8 px (inside the ramp's linear zone): rho' far from 1, rho'' far from 0"""
    xy = np.array(prob["obs_xy"])
    xy[::9] += np.array([6.0, -5.0])
    return geom_cases.as_ramp_problem(prob, xy)


def _single_observation_point(prob, point):
    keep = np.asarray(prob["obs_point"]) != point
    keep[np.flatnonzero(~keep)[0]] = True
    out = dict(prob)
    for key in ("obs_image", "obs_point", "obs_xy"):
        out[key] = np.ascontiguousarray(np.asarray(prob[key])[keep])
    return geom_cases.as_ramp_problem(out, out["obs_xy"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, loss, gauge, singular points) by name; built once"""
    singular = []
    loss = TRIVIAL
    if name == "wide":            # one 12-parameter camera (THIN_PRISM_FISHEYE) shared by all images, every intrinsic variable: dc = 18
        prob = geom_cases.make_model_case(10, n_cams=6, n_points=40, obs_per_point=4, seed=11, shared_camera=True)
        gauge = _gauge(prob, cam_const=0)
    elif name == "thirty":        # n_c = 28 * 6 + 30 * 2 = 228: four tiles of the dense inverse (60 points in 6 images each: 12 observations per image)
        prob = geom_cases.make_case(n_cams=30, n_points=60, obs_per_point=6, seed=12)
        gauge = _gauge(prob)
    else:
        prob = geom_cases.make_case(n_cams=6, n_points=40, obs_per_point=4, seed=10)
        gauge = _gauge(prob)
        if name == "cauchy":
            prob, loss = _with_outliers(prob), CAUCHY
        elif name == "tvec_mask":
            gauge[1][3] = 0b101
        elif name == "quarter_const":
            gauge[3][::4] = 1
        elif name == "points_const":
            gauge[3][:] = 1
        elif name == "cameras_const":
            gauge[0][:] = 1
            gauge[2][:] = 0xfff
        elif name == "single_obs":
            prob = _single_observation_point(prob, 7)
            singular = [7]
        else:
            assert name == "trivial", name
    return prob, loss, tuple(gauge), tuple(singular)


CASES = ["trivial", "cauchy", "wide", "tvec_mask", "quarter_const", "points_const", "cameras_const", "thirty", "single_obs"]


# ---- reference ------------------------------------------------------------------------------------------------------------------------
def corrected_jacobian(prob, loss, gauge, r, J, singular=()):
    """(J~ (n_obs * C, n_var) long double, columns dict, point columns {point: first column}) from the oracle's raw blocks"""
    import pxo
    from pixsfm_amd.engine import column_layout
    pose_const, tmask, cmask, ptc = gauge
    cols = column_layout(pose_const, tmask, cmask, prob["cam_model"])
    n_obs, C = r.shape
    seen = np.zeros(len(prob["xyz"]), bool)
    seen[np.asarray(prob["obs_point"])] = True
    pt_col, n_var = {}, cols["n_c"]
    for p in range(len(prob["xyz"])):
        if seen[p] and not ptc[p] and p not in singular:
            pt_col[p] = n_var
            n_var += 3
    Jt = np.zeros((n_obs * C, n_var), LD)
    ls = pxo.loss(*loss)
    for i in range(n_obs):
        img, pt = int(prob["obs_image"][i]), int(prob["obs_point"][i])
        cam = int(prob["image_camera"][img])
        ri, Ji = r[i].astype(LD), J[i].astype(LD)
        s = float(ri @ ri)
        rho = pxo.loss_eval(ls, s)
        Jc = Ji * np.sqrt(LD(rho[1]))
        if s != 0.0 and rho[2] > 0.0:
            alpha = 1.0 - np.sqrt(LD(1.0) + 2.0 * s * LD(rho[2]) / LD(rho[1]))
            Jc = np.sqrt(LD(rho[1])) * (Ji - (alpha / s) * np.outer(ri, ri @ Ji))
        rows = slice(i * C, (i + 1) * C)
        q = np.asarray(prob["qvec"][img], dtype=LD)
        PJ = np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]], dtype=LD)
        tangent = np.concatenate([Jc[:, 0:4] @ PJ, Jc[:, 4:7]], axis=1)              # (rotation, tx, ty, tz)
        for a, slot in enumerate(cols["pose_slots"][img]):
            Jt[rows, cols["pose_off"][img] + a] = tangent[:, slot]
        for a, k in enumerate(cols["intr_slots"][cam]):
            Jt[rows, cols["intr_off"][cam] + a] = Jc[:, 10 + k]
        if pt in pt_col:
            Jt[rows, pt_col[pt]:pt_col[pt] + 3] = Jc[:, 7:10]
    return Jt, cols, pt_col


class Reference:
    """H, its factor and inverse in long double; numpy's float64 inverse of the float64 H; the blocks' index sets"""

    def __init__(self, prob, loss, gauge, r, J, cost, singular=()):
        Jt, self.cols, self.pt_col = corrected_jacobian(prob, loss, gauge, r, J, singular)
        self.n_c, self.n_obs, self.cost = self.cols["n_c"], len(r), cost
        H = Jt.T @ Jt
        self.L, _, self.Sigma = sic.reference(H)
        J64 = Jt.astype(np.float64)
        self.Sigma_np = np.linalg.inv(J64.T @ J64)
        # the scaled matrix of the quantum term: camera columns into [1/4, 1) by powers of two
        d = np.ones(H.shape[0])
        for c in range(self.n_c):
            e = np.frexp(float(H[c, c]))[1]
            d[c] = np.ldexp(1.0, (-e) >> 1)
        Hs = (H * d[:, None] * d[None, :]).astype(np.float64)
        self.lambda_min = float(np.linalg.eigvalsh(Hs)[0])

    def whitened(self, index, block, sigma=None):
        """max |L^T Delta L| for Delta = block - Sigma_ref[index, index]"""
        index = np.asarray(index, dtype=np.int64)
        if len(index) == 0:
            return 0.0
        ref = (self.Sigma if sigma is None else sigma)[np.ix_(index, index)]
        W = self.L[index, :]
        return float(np.abs(W.T @ (np.asarray(block).astype(LD) - ref) @ W).max())

    def quantum_term(self):
        if self.n_c == 0:
            return 0.0
        q = 2.0 ** (int(np.ceil(np.log2(max(1.0, 4.0 * np.sqrt(self.cost))))) - 62)
        return 4.0 * self.n_c * self.n_obs * q / self.lambda_min


def blocks_of(ref, prob, cov):
    """[(name, global index set, the device's block restricted to the variable components, reference exists)]"""
    out = []
    cols = ref.cols
    for img, slots in enumerate(cols["pose_slots"]):
        idx = [cols["pose_off"][img] + a for a in range(len(slots))]
        out.append(("pose %d" % img, idx, cov["pose"][img][np.ix_(slots, slots)]))
    for cam, slots in enumerate(cols["intr_slots"]):
        idx = [cols["intr_off"][cam] + a for a in range(len(slots))]
        out.append(("intrinsics %d" % cam, idx, cov["intrinsics"][cam][np.ix_(slots, slots)]))
    for p, c0 in ref.pt_col.items():
        out.append(("point %d" % p, [c0, c0 + 1, c0 + 2], cov["points"][p]))
    if "cameras" in cov and ref.n_c > 0:
        out.append(("cameras", list(range(ref.n_c)), cov["cameras"]))
    return out


def check_against_reference(tag, ref, prob, gauge, cov, singular=()):
    pose_const, tmask, cmask, ptc = gauge
    assert cov["summary"]["info"] == 0, cov["summary"]
    assert cov["summary"]["num_camera_unknowns"] == ref.n_c
    assert cov["summary"]["num_singular_points"] == len(singular)
    worst = worst_np = worst_fro = 0.0
    for name, idx, block in blocks_of(ref, prob, cov):
        assert np.all(np.isfinite(block)), name
        e = ref.whitened(idx, block)
        e_np = ref.whitened(idx, ref.Sigma_np[np.ix_(idx, idx)])
        want = ref.Sigma[np.ix_(idx, idx)].astype(np.float64) if len(idx) else np.zeros((0, 0))
        fro = float(np.linalg.norm(block - want) / np.linalg.norm(want)) if len(idx) else 0.0
        worst, worst_np, worst_fro = max(worst, e), max(worst_np, e_np), max(worst_fro, fro)
        assert fro <= 1e-6, (tag, name, fro)
    bound = 64.0 * worst_np + ref.quantum_term()
    print("%s: n_c %d, whitened error %.3g (numpy %.3g, quantum term %.3g, bound %.3g), worst block Frobenius %.3g"
          % (tag, ref.n_c, worst, worst_np, ref.quantum_term(), bound, worst_fro))
    assert worst <= bound, (tag, worst, bound)
    # constant parameters: zero rows and columns, exactly
    for img, slots in enumerate(ref.cols["pose_slots"]):
        const = [k for k in range(6) if k not in slots]
        assert not cov["pose"][img][const, :].any() and not cov["pose"][img][:, const].any(), img
    for cam, slots in enumerate(ref.cols["intr_slots"]):
        const = [k for k in range(cov["intrinsics"].shape[1]) if k not in slots]
        assert not cov["intrinsics"][cam][const, :].any() and not cov["intrinsics"][cam][:, const].any(), cam
    for p in range(len(prob["xyz"])):
        if p in singular:
            assert np.isnan(cov["points"][p]).all(), p
        elif p not in ref.pt_col:
            assert not cov["points"][p].any(), p
        else:
            assert np.array_equal(cov["points"][p], cov["points"][p].T), p


def geometric_covariance(ctx, prob, loss, gauge, cameras=True):
    from pixsfm_amd.engine import GeometricBAProblem, make_loss
    ba = GeometricBAProblem(ctx, geom_cases.geometric_dict(prob))
    ba.eval(residuals=False)
    return ba.covariance(make_loss(loss[0], [loss[1]]), *gauge, cameras=cameras)


@functools.lru_cache(maxsize=None)
def reference(name):
    prob, loss, gauge, singular = case(name)
    cost, r, J = geom_cases.oracle_eval(prob, loss, want_J=True)
    return Reference(prob, loss, gauge, r, J[:, :2, :], cost, singular)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_blocks_match_the_inverse_of_the_oracles_normal_matrix(ctx, name):
    prob, loss, gauge, singular = case(name)
    cov = geometric_covariance(ctx, prob, loss, gauge)
    check_against_reference(name, reference(name), prob, gauge, cov, singular)
    if name == "cameras_const":        # Sigma_p = inv(V_p) exactly as the 3 x 3 Cholesky gives it: no camera term was added
        assert cov["summary"]["num_camera_unknowns"] == 0 and "cameras" in cov and cov["cameras"].shape == (0, 0)
    if name == "points_const":
        assert not cov["points"].any()


def test_featuremetric_records(ctx):
    """records of BAProblem.eval (the exact-order kernel on float64 ramp patches, three channels -- pxr_ba_eval takes 1, 3, 64 or
    128 -- of which the third is zero, l2_normalize off, zero references) instead of the geometric kernel's"""
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, make_loss
    base, loss, gauge, _ = case("cauchy")
    prob = geom_cases.as_ramp_problem(base, base["obs_xy"], channels=3)
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ba = BAProblem(ctx, arena, prob)
    ba.eval(interp_cfg(l2_normalize=False), with_jacobian=True)
    cov = ba.covariance(make_loss(loss[0], [loss[1]]), *gauge, cameras=True)
    arena.close()
    check_against_reference("featuremetric", reference("cauchy"), prob, gauge, cov)


def test_no_gauge_is_reported_not_inverted(ctx):
    """every pose, camera and point variable: S has the seven-dimensional gauge null space -- an ordinary return with info > 0"""
    prob, loss, gauge, _ = case("trivial")
    free = (np.zeros_like(gauge[0]), gauge[1], gauge[2], gauge[3])
    cov = geometric_covariance(ctx, prob, loss, free)
    info = cov["summary"]["info"]
    print("no gauge: info %d of n_c %d" % (info, cov["summary"]["num_camera_unknowns"]))
    assert 0 < info <= cov["summary"]["num_camera_unknowns"]


@pytest.mark.parametrize("name", ["cauchy", "thirty"])
def test_two_calls_give_the_same_bits(ctx, name):
    prob, loss, gauge, _ = case(name)
    a, b = geometric_covariance(ctx, prob, loss, gauge), geometric_covariance(ctx, prob, loss, gauge)
    for key in ("pose", "intrinsics", "points", "cameras"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_the_view_is_not_written(ctx):
    from pixsfm_amd.engine import GeometricBAProblem, make_loss
    prob, loss, gauge, _ = case("trivial")
    ba = GeometricBAProblem(ctx, geom_cases.geometric_dict(prob))
    before = [a.tobytes() for a in ba.params()]
    ba.eval(residuals=False)
    ba.covariance(make_loss(*TRIVIAL[:1], [1.0]), *gauge)
    assert before == [a.tobytes() for a in ba.params()]


def test_existing_geometric_solve_keeps_its_bits(ctx):
    """the solver shares its linearisation with the covariance: a six-iteration pxr_ba_solve_geometric gives the bits recorded
    before the covariance was added (tests/golden/ba_geom_solve_bits.npz)"""
    from pixsfm_amd.engine import GeometricBAProblem, lm_options, make_loss
    prob = geom_cases.make_case(n_cams=6, n_points=40, obs_per_point=4, seed=3, model=2, ramp=False)
    n_img, n_cam, n_pt = len(prob["image_camera"]), len(prob["cam_model"]), len(prob["xyz"])
    pose_const = np.zeros(n_img, np.uint8)
    pose_const[:2] = 1
    ba = GeometricBAProblem(ctx, geom_cases.geometric_dict(prob))
    s = ba.solve(make_loss("cauchy", [1.0]), pose_const, np.zeros(n_img, np.uint8), np.zeros(n_cam, np.uint16), np.zeros(n_pt, np.uint8),
                 options=lm_options(max_iterations=6, linear_solver="direct"))
    want = np.load(GOLDEN)
    assert s["iterations"] == int(want["iterations"]) and s["final_cost"] == float(want["final_cost"])
    for got, key in zip(ba.params(), ("qvec", "tvec", "cam_params", "xyz")):
        assert got.tobytes() == want[key].tobytes(), key


def test_api_by_strategy_scale_and_missing_gauge(ctx):
    """estimate_ba_covariance on a reconstruction: the bundle adjusters' default gauge (first pose constant, tx of the second),
    the posterior scale, and the ValueError of a setup that fixes nothing"""
    from pixsfm_amd import synthetic
    from pixsfm_amd.api import BundleAdjustmentSetup, estimate_ba_covariance
    from pixsfm_amd.api.reconstruction import reconstruction_from_flat
    flat = synthetic.make_ba_problem(n_cams=5, n_points=50, obs_per_point=4, seed=21, channels=1, patch_size=2)
    rec, _ = reconstruction_from_flat(flat, keypoint_noise=0.5)
    ids = rec.reg_image_ids()
    unit = estimate_ba_covariance({"strategy": "geometric"}, rec)
    assert not unit.pose_cov(ids[0]).any()
    second = unit.pose_cov(ids[1])
    assert not second[3].any() and not second[:, 3].any() and np.linalg.eigvalsh(np.delete(np.delete(second, 3, 0), 3, 1))[0] > 0
    for i in ids[2:]:
        assert np.linalg.eigvalsh(unit.pose_cov(i))[0] > 0
    p = rec.point3D_ids()[0]
    assert np.linalg.eigvalsh(unit.point_cov(p))[0] > 0
    dense, names = unit.cameras_cov()
    k = names.index(("pose", ids[2], 0))
    assert np.array_equal(dense[k:k + 6, k:k + 6], unit.pose_cov(ids[2]))
    post = estimate_ba_covariance({"strategy": "geometric"}, rec, scale="posterior")
    s = post.summary
    assert s["factor"] == 2.0 * s["cost"] / (s["num_residuals"] - s["num_parameters"])
    assert s["num_residuals"] == 2 * rec.num_observations()
    assert np.array_equal(post.pose_cov(ids[2]), unit.pose_cov(ids[2]) * s["factor"])
    free = BundleAdjustmentSetup()
    free.add_images(ids)
    with pytest.raises(ValueError, match="gauge is not fixed"):
        estimate_ba_covariance({"strategy": "geometric"}, rec, free)
