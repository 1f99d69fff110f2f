"""Cases, a long-double reference and a DERIVED error bound for the Gram-matrix evaluation of the feature-reference residual
(csrc/pxr_gram.h, csrc/pxr_ba_gram.hip).  No GPU in this module: tests/test_gram_reference_cpu.py checks it against itself and
the oracle, tests/test_gram_records_gpu.py holds pxr_ba_eval_gram to it.

THE OPERATION (`reference_record`).  u = x sx - 0.5 - cx, v = y sy - 0.5 - cy in fp64 (what the device computes: with the
power-of-two patch scales of every case here x sx is exact, so the value is the same with and without FMA contraction); the cell
is floor(u), floor(v) limited to [-3, n + 1] like texel_index, every tap of the 4 x 4 stencil is clamped into the patch on its
own like GramTexels::load, the fractions u - floor(u), v - floor(v) are the fp64 differences the device forms.  From there on
everything is np.longdouble (64-bit significand: 2^-11 of an fp64 rounding per operation) and written per channel, without G:
Catmull-Rom weights and derivatives, f = w.T, fc, fr, the L2 normalisation with its chain rule, r = fh - d and the six record
entries  |r|^2, fc.fc sx^2, fc.fr sx sy, fr.fr sy^2, fc.r sx, fr.r sy.

THE SECOND STATEMENT (`restated_record`): the algebra of pxr_gram.h in numpy float64 -- G = T T^t, D = T d, the nine forms in
the grouping of gram_rows_times_weights / gram_eval_eight (4-term sums over the horizontal taps, 4-term sums over the vertical
taps, a 16-term sum over the rows as pairs and a three-level tree) and the two epilogues.

THE BOUND (`bound`): per observation and entry  K * 2^-53 * scale.  With A = |w|_1, B = max(|wc|_1, |wr|_1), tau = the largest
channel norm of the 16 stencil texels, rho = |d|, N = |f| (all from the reference):
    l2 off:  |r|^2: (A tau + rho)^2      Gram: (B tau)^2 s_a s_b         J^t r: B tau (A tau + rho) s_a
    l2 on :  |r|^2: (kappa + rho)^2      Gram: beta^2 kappa^2 s_a s_b    J^t r: beta kappa (kappa + rho) s_a
             kappa = A tau / N >= 1,  beta = B tau / N.

K, counted (first order in u = 2^-53; every count is a worst case, |x (1 + d)| with |d| <= u per rounding):
 0. Inputs.  Texels, reference descriptor and the two fractions are the same numbers on both sides: no error.
 1. 1-D weights.  x2 = x x carries 1u, x3 = x2 x 2u (relative).  Each tap is a sum of at most three terms c x^k; charging every
    product its relative error times its largest magnitude on [0, 1) and every addition u times its largest partial sum:
        w :  2.6 + 12 + 10 + 1.6  <= 27 u   (taps 0..3; e.g. tap 1 = 1 - 2.5 x2 + 1.5 x3: 5 + 1.5 + 4.5 + 1)
        w':  5 + 15.4 + 14.9 + 3.5 <= 39 u  (e.g. tap 1 = -5 x + 4.5 x2: 5 + 9 + 1.4)
    in the 1-norm over the four taps (an FMA only removes roundings).  |w_1d|_1 <= 1.25, |w'_1d|_1 <= 3, so for the Kronecker
    products  |dw|_1 <= 2 * 1.25 * 27 u = 67.5 u =: e_w u  and  |dwc|_1, |dwr|_1 <= (3 * 27 + 1.25 * 39) u <= 130 u =: e_d u.
    The taps of w sum to 1 and |w'_1d|_1 >= 1, so A >= 1 and B >= 1: the two are also relative to A and B.
 2. Contractions over the C channels, in any order, with or without FMA:  |dG_ij| <= C u tau^2,  |dD_i| <= C u tau rho,
    |d(d.d)| <= C u rho^2  (fp16 x fp16 and fp32 x fp32 products are exact in fp64).
 3. A form a^t G b:  4-term sum over the horizontal taps (4u), 4-term sum over the vertical taps (4u), the product of the two
    1-D weights of a row (1u), the pair of rows (2u), three levels of the 8-lane sum (3u): 14u of sum |a_i| |G_ij| |b_j|
    <= tau^2 |a|_1 |b|_1.  A linear form a.D: 1 + 2 + 3 = 6u.  Together with 1. and 2.
        d(a^t G b) <= (C + 14 + e_a + e_b) u tau^2 |a|_1 |b|_1      d(a.D) <= (C + 6 + e_a) u tau rho |a|_1
        e_gg = C + 149   e_gc = C + 211.5   e_cc = C + 274   e_fd = C + 73.5   e_cd = C + 136
 4. Epilogue without normalisation.  s = Sgg - 2 Sfd + d.d: e_gg (A tau)^2 + 2 e_fd A tau rho + C rho^2 + 2 additions of
    partial sums <= (A tau + rho)^2:  C + 151.  A Gram entry: e_cc + 2 multiplications by the scales:  C + 276.
    J^t r = (Sgc - Scd) s: e_gc A B tau^2 + e_cd B tau rho + subtraction + scale:  C + 213.5.
        K(C, l2 off) = C + 276                                                  (404 at C = 128, 340 at C = 64)
 5. Epilogue with normalisation (the cases keep rho <= 1).  Sgg / N^2 has the relative error e_gg kappa^2 u; 1 / sqrt(Sgg)
    half of it + 2u, its square e_gg kappa^2 + 5.
    s = 1 - 2 Sfd / N + d.d:  2 e_fd kappa rho + (e_gg kappa^2 + 6) rho + C rho^2 + 2 additions  <=  (C + 154) (kappa + rho)^2.
    gcc = (Scc - Sgc pc) / N^2, pc = Sgc / N^2, every term <= beta^2:  e_cc + 2 kappa e_gc (Sgc twice) + 2 kappa^2 e_gg (1 / N^2
    inside pc and outside) + 16 roundings of the epilogue and the scales  <=  (5 C + 1011) beta^2 kappa^2.
    bc = -(Scd - Sfd pc) / N, every term <= beta rho:  e_cd + kappa (e_fd + e_gc) + 1.5 kappa^2 e_gg + 13; the kappa^2 part is
    <= 1.5 e_gg beta kappa^2 (rho <= 1), the rest <= (3 C + 434) beta kappa rho:  3 C + 434 of beta kappa (kappa + rho).
        K(C, l2 on) = 5 C + 1011                                                (1651 at C = 128, 1331 at C = 64)
This is more than "C plus a few tens": the weights are charged their polynomial coefficients (up to 5) instead of one rounding
each, and the normalised Gram entry sums three forms that share N.  It is a worst case, not a fit: the float64 restatement
stays near 7 * 2^-53 * scale (tests/test_gram_reference_cpu.py prints it), i.e. the bound has two orders of head room and is
still more than four orders below FP32_PASS_RECORD_ATOL on the unit-norm cases (asserted there).
"""
import functools

import numpy as np

H, W = 7, 9                      # non-square on purpose: a row / column swap moves every stencil
U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double with a 64-bit significand"
E_W1, E_D1 = 27.0, 39.0          # 1-norm rounding of the four 1-D weights / derivative weights, in u (item 1)
BATCH_SIZES = (1, 7, 8, 9, 63, 64, 65, 200)


def K(C, l2):
    return 5 * C + 1011 if l2 else C + 276


# ---- the operation ------------------------------------------------------------------------------------------------------------
def catmull_rom(x, dt):
    """Weights of the four taps at fraction x and their derivatives, in precision dt (the polynomials of pxr_gram.h)."""
    x = dt(x)
    x2 = x * x
    x3 = x2 * x
    h, one = dt(0.5), dt(1.0)
    w = [-h * x + x2 - h * x3, one - dt(2.5) * x2 + dt(1.5) * x3, h * x + dt(2.0) * x2 - dt(1.5) * x3, -h * x2 + h * x3]
    dw = [-h + dt(2.0) * x - dt(1.5) * x2, -dt(5.0) * x + dt(4.5) * x2, h + dt(4.0) * x - dt(4.5) * x2, -x + dt(1.5) * x2]
    return np.array(w, dtype=dt), np.array(dw, dtype=dt)


def stencil(xy, scale, corner):
    """fp64, like the device: (row, col) of the cell limited as texel_index does, the fractions, the clamped tap rows / cols."""
    u = np.float64(xy[0]) * np.float64(scale[0]) - 0.5 - np.float64(corner[0])
    v = np.float64(xy[1]) * np.float64(scale[1]) - 0.5 - np.float64(corner[1])
    cf, rf = np.floor(u), np.floor(v)
    col, row = int(min(max(cf, -3.0), W + 1.0)), int(min(max(rf, -3.0), H + 1.0))
    rows = np.clip(row - 1 + np.arange(4), 0, H - 1)
    cols = np.clip(col - 1 + np.arange(4), 0, W - 1)
    return row, col, u - cf, v - rf, rows, cols


def _texels(patch, rows, cols, dt):
    """(16, C): texel t = 4 * (vertical tap) + (horizontal tap), exact in dt."""
    return patch[rows][:, cols].reshape(16, patch.shape[-1]).astype(dt)


def reference_record(patch, d, xy, scale, corner, l2):
    """The six record entries in long double, per channel, and the quantities the bound is made of."""
    _, _, fu, fv, rows, cols = stencil(xy, scale, corner)
    T = _texels(patch, rows, cols, LD)
    d = np.asarray(d).astype(LD)
    sx, sy = LD(scale[0]), LD(scale[1])
    wu, dwu = catmull_rom(fu, LD)
    wv, dwv = catmull_rom(fv, LD)
    w, wc, wr = np.outer(wv, wu).ravel(), np.outer(wv, dwu).ravel(), np.outer(dwv, wu).ravel()
    f, fc, fr = (w[:, None] * T).sum(0), (wc[:, None] * T).sum(0), (wr[:, None] * T).sum(0)
    N = np.sqrt((f * f).sum())
    fh = f
    if l2:
        fh = f / N
        fc = (fc - fh * (fh * fc).sum()) / N
        fr = (fr - fh * (fh * fr).sum()) / N
    r = fh - d
    rec = np.array([(r * r).sum(), (fc * fc).sum() * sx * sx, (fc * fr).sum() * sx * sy, (fr * fr).sum() * sy * sy,
                    (fc * r).sum() * sx, (fr * r).sum() * sy], dtype=LD)
    q = dict(A=np.abs(w).sum(), B=max(np.abs(wc).sum(), np.abs(wr).sum()), tau=np.sqrt((T * T).sum(1)).max(),
             rho=np.sqrt((d * d).sum()), N=N)
    return rec, q


def bound(q, scale, l2, C):
    """K * 2^-53 * scale for the six entries (module docstring)."""
    sx, sy = LD(scale[0]), LD(scale[1])
    if l2:
        kappa, beta = q["A"] * q["tau"] / q["N"], q["B"] * q["tau"] / q["N"]
        s0, g, j = (kappa + q["rho"]) ** 2, (beta * kappa) ** 2, beta * kappa * (kappa + q["rho"])
    else:
        at, bt = q["A"] * q["tau"], q["B"] * q["tau"]
        s0, g, j = (at + q["rho"]) ** 2, bt ** 2, bt * (at + q["rho"])
    return LD(K(C, l2) * U) * np.array([s0, g * sx * sx, g * sx * sy, g * sy * sy, j * sx, j * sy], dtype=LD)


def _sum16(p):
    """Rows in pairs, then the three levels of the 8-lane sum."""
    s = p[0::2] + p[1::2]
    s = s[0::2] + s[1::2]
    s = s[0::2] + s[1::2]
    return s[0] + s[1]


def restated_record(patch, d, xy, scale, corner, l2):
    """The algebra of pxr_gram.h in float64."""
    _, _, fu, fv, rows, cols = stencil(xy, scale, corner)
    T = _texels(patch, rows, cols, np.float64)
    d = np.asarray(d, dtype=np.float64)
    sx, sy = float(scale[0]), float(scale[1])
    G, D, r2 = T @ T.T, T @ d, float(d @ d)
    wu, dwu = catmull_rom(fu, np.float64)
    wv, dwv = catmull_rom(fv, np.float64)
    Gb = G.reshape(16, 4, 4)                                   # [row i][vertical tap][horizontal tap]
    z, zc = (Gb * wu).sum(-1), (Gb * dwu).sum(-1)              # gram_rows_times_weights: over the horizontal taps ...
    y, yc, yr = (z * wv).sum(-1), (zc * wv).sum(-1), (z * dwv).sum(-1)      # ... then the vertical ones: G w, G wc, G wr
    om, omc, omr = np.outer(wv, wu).ravel(), np.outer(wv, dwu).ravel(), np.outer(dwv, wu).ravel()
    Sgg, Sgc, Sgr = _sum16(om * y), _sum16(om * yc), _sum16(om * yr)
    Scc, Scr, Srr = _sum16(omc * yc), _sum16(omc * yr), _sum16(omr * yr)
    Sfd, Scd, Srd = _sum16(om * D), _sum16(omc * D), _sum16(omr * D)
    if l2:
        ninv = 1.0 / np.sqrt(Sgg)
        n2inv = ninv * ninv
        pc, pr = Sgc * n2inv, Sgr * n2inv
        s = 1.0 - 2.0 * Sfd * ninv + r2
        gcc, gcr, grr = (Scc - Sgc * pc) * n2inv, (Scr - Sgc * pr) * n2inv, (Srr - Sgr * pr) * n2inv
        bc, br = -(Scd - Sfd * pc) * ninv, -(Srd - Sfd * pr) * ninv
    else:
        s = Sgg - 2.0 * Sfd + r2
        gcc, gcr, grr, bc, br = Scc, Scr, Srr, Sgc - Scd, Sgr - Srd
    s = max(s, 0.0)
    return np.array([s, gcc * sx * sx, gcr * sx * sy, grr * sy * sy, bc * sx, br * sy])


def oracle_record(patch, d, xy, scale, corner, l2):
    """The same six entries from the oracle's PatchInterpolator (fp32 horizontal pass), formed the same way."""
    import pxo
    p = pxo.make_patch(np.ascontiguousarray(patch), corner, scale)
    f, gx, gy, _ = pxo.patch_eval(p, np.asarray(xy, dtype=np.float64), pxo.cfg(l2_normalize=bool(l2)))
    r = f - np.asarray(d, dtype=np.float64)
    return np.array([r @ r, gx @ gx, gx @ gy, gy @ gy, gx @ r, gy @ r])


def closed_form_on_a_texel(patch, d, row, col, scale, l2):
    """Fractions exactly 0 in u and v: f is the texel (row, col), the derivatives are central differences of its neighbours."""
    P = patch.astype(LD)
    cl = lambda r, c: P[min(max(r, 0), H - 1), min(max(c, 0), W - 1)]
    f = cl(row, col)
    fc, fr = (cl(row, col + 1) - cl(row, col - 1)) / 2, (cl(row + 1, col) - cl(row - 1, col)) / 2
    if l2:
        N = np.sqrt((f * f).sum())
        f = f / N
        fc, fr = (fc - f * (f * fc).sum()) / N, (fr - f * (f * fr).sum()) / N
    r = f - np.asarray(d).astype(LD)
    sx, sy = LD(scale[0]), LD(scale[1])
    return np.array([(r * r).sum(), (fc * fc).sum() * sx * sx, (fc * fr).sum() * sx * sy, (fr * fr).sum() * sy * sy,
                     (fc * r).sum() * sx, (fr * r).sum() * sy], dtype=LD)


def evaluate(group, xy, fn=reference_record):
    """fn on every observation of a group at the pixel positions xy (n, 2)."""
    p = group["prob"]
    out = []
    for o in range(len(xy)):
        k = int(p["obs_patch"][o])
        out.append(fn(p["patches"][k], p["refs"][p["obs_point"][o]], xy[o], p["scales"][k], p["corners"][k], group["l2"]))
    return out


def reference_and_bound(group, xy):
    """(n, 6) reference records and bounds, both long double."""
    res = evaluate(group, xy)
    p = group["prob"]
    bnd = [bound(q, p["scales"][int(p["obs_patch"][o])], group["l2"], group["C"]) for o, (_, q) in enumerate(res)]
    return np.stack([r for r, _ in res]), np.stack(bnd)


# ---- host projection (fp64; the GPU tests take the device's own x, y instead) ---------------------------------------------------
def host_xy(prob):
    """WorldToPixel for the three camera models the cases use (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL)."""
    out = np.empty((len(prob["obs_image"]), 2))
    for o, (i, j) in enumerate(zip(prob["obs_image"], prob["obs_point"])):
        q = prob["qvec"][i] / np.linalg.norm(prob["qvec"][i])
        X = prob["xyz"][j]
        uv = 2.0 * np.cross(q[1:], X)
        p = X + q[0] * uv + np.cross(q[1:], uv) + prob["tvec"][i]
        a, b = p[0] / p[2], p[1] / p[2]
        cam = prob["image_camera"][i]
        m, k = prob["cam_model"][cam], prob["cam_params"][cam]
        if m == 0:
            out[o] = k[0] * a + k[1], k[0] * b + k[2]
        elif m == 1:
            out[o] = k[0] * a + k[2], k[1] * b + k[3]
        else:
            assert m == 2
            rad = k[3] * (a * a + b * b)
            out[o] = k[0] * (a + a * rad) + k[1], k[0] * (b + b * rad) + k[2]
    return out


# ---- content --------------------------------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def smooth_features(rng, n, C):
    """(f) low-frequency waves over the patch with a phase per channel, every texel of unit norm (before the storage rounding)."""
    r, c = np.arange(H)[None, :, None, None], np.arange(W)[None, None, :, None]
    a, b = rng.uniform(-0.6, 0.6, (2, n, 1, 1, C))
    return _unit(np.sin(a * r + b * c + rng.uniform(0, 2 * np.pi, (n, 1, 1, C))) + 0.3)


def noise_features(rng, n, C):
    """(g) white noise, texel norms around 1."""
    return rng.normal(0.0, 1.0, (n, H, W, C)) / np.sqrt(C)


def _references(rng, patches, obs_patch, obs_point, n_points):
    """A unit-norm reference per point: the centre texel of one of its observations' patches, perturbed."""
    C = patches.shape[-1]
    refs = np.empty((n_points, C))
    for o in range(len(obs_patch)):
        refs[obs_point[o]] = patches[obs_patch[o], H // 2, W // 2].astype(np.float64)
    return _unit(_unit(refs) + rng.normal(0, 0.3 / np.sqrt(C), refs.shape))


# ---- problems -------------------------------------------------------------------------------------------------------------------
PATCH_FRAMES = [((1.0, 1.0), (0, 0)), ((0.25, 2.0), (-3, 5)), ((1.0, 0.5), (4, -2))]     # (e): (scale, corner), powers of two


def placed_problem(uv, frames, patches, refs=None, rng=None, twins=()):
    """One observation per image, camera, point and patch; SIMPLE_PINHOLE f = 1, c = 0, identity pose, X = (x, y, 1): the pixel is
    X[:2] exactly, and with power-of-two scales the patch coordinate is the planned (u, v) exactly.  Observation o reads patch
    perm[o] (a permutation: obs_patch is not the identity).  twins: pairs (o, o2), o2 gets a copy of o's patch and reference."""
    n = len(uv)
    rng = rng or np.random.default_rng(n)
    perm = rng.permutation(n)
    for o, o2 in twins:
        patches[perm[o2]] = patches[perm[o]]
    scales, corners = np.empty((n, 2)), np.empty((n, 2), np.int32)
    xy = np.empty((n, 2))
    for o in range(n):
        s, c = frames[o % len(frames)]
        scales[perm[o]], corners[perm[o]] = s, c
        xy[o] = (uv[o] + 0.5 + np.asarray(c, np.float64)) / np.asarray(s)
        assert np.array_equal(xy[o] * np.asarray(s) - 0.5 - np.asarray(c, np.float64), uv[o]), "the planned position is not exact"
    ids = np.arange(n, dtype=np.int32)
    if refs is None:
        refs = _references(rng, patches, perm, ids, n)
        for o, o2 in twins:
            refs[o2] = refs[o]
    prob = dict(obs_image=ids, obs_point=ids, obs_patch=perm.astype(np.int64), image_camera=ids,
                qvec=np.tile([1.0, 0, 0, 0], (n, 1)), tvec=np.zeros((n, 3)), cam_model=np.zeros(n, np.int32),
                cam_params=np.tile([1.0, 0.0, 0.0], (n, 1)), xyz=np.column_stack([xy, np.ones(n)]), refs=refs,
                patches=patches, corners=corners, scales=scales)
    return prob, xy


def shared_problem(rng, n_obs, patches):
    """Shared patches (obs_patch has repeats and is permuted), several observations per point, five images over a PINHOLE and a
    SIMPLE_RADIAL camera whose focal lengths keep every projection within a texel or two of the 7 x 9 patch."""
    n_patches = len(patches)
    n_img, n_pts = 5, max(1, n_obs // 3)
    obs_point = (np.arange(n_obs) % n_pts).astype(np.int32)
    obs_image = rng.integers(0, n_img, n_obs).astype(np.int32)
    obs_patch = rng.integers(0, n_patches, n_obs).astype(np.int64)
    z = rng.uniform(4.0, 6.0, n_pts)
    xyz = np.column_stack([rng.uniform(-1.3, 1.3, n_pts) * z, rng.uniform(-1.3, 1.3, n_pts) * z, z])
    qvec = np.column_stack([np.ones(n_img), rng.normal(0, 0.02, (n_img, 3))])
    corners = np.zeros((n_patches, 2), np.int32)
    corners[1::3] = (1, -1)
    corners[2::3] = (-1, 0)
    return dict(obs_image=obs_image, obs_point=obs_point, obs_patch=obs_patch, image_camera=np.array([0, 1, 0, 1, 1], np.int32),
                qvec=qvec, tvec=rng.normal(0, 0.1, (n_img, 3)), cam_model=np.array([1, 2], np.int32),
                cam_params=np.array([[3.5, 2.5, 4.5, 3.5], [3.0, 4.5, 3.5, 0.05]]), xyz=xyz,
                refs=_references(rng, patches, obs_patch, obs_point, n_pts), patches=patches, corners=corners,
                scales=np.ones((n_patches, 2)))


def planned_positions():
    """(a)-(d) as patch coordinates (u, v), with what each is: a list of (u, v, tag)."""
    out = []
    out += [(3.0, 2.375, "a:u"), (3.40625, 2.0, "a:v"), (3.0, 2.0, "a:uv"), (0.0, 0.0, "a:uv"), (W - 1.0, H - 1.0, "a:uv")]
    e = 1.0 - 2.0 ** -30
    out += [(3.0 + e, 2.5, "b"), (3.25, 2.0 + e, "b"), (5.0 + e, 4.0 + e, "b")]
    # (c) cells -2 (3 taps clamped), -1 (2), 0 (1), interior, n - 2 (1), n - 1 (2), n (3) in each direction: every border and corner
    us = [c + 0.375 for c in (-2, -1, 0, 4, W - 2, W - 1, W)]
    vs = [r + 0.625 for r in (-2, -1, 0, 3, H - 2, H - 1, H)]
    out += [(u, v, "c") for v in vs for u in us]
    # (d) 50 texels outside, each followed by the position with the same fraction at the limit of the cell index
    out += [(-50.625, 2.25, "d"), (-2.625, 2.25, "d="), (W + 50.375, 2.25, "d"), (W + 1.375, 2.25, "d="),
            (3.25, -50.875, "d"), (3.25, -2.875, "d="), (3.25, H + 50.125, "d"), (3.25, H + 1.125, "d=")]
    return out


def _group(name, C, dtype, l2, prob, planned=None, tags=None):
    prob["patches"] = np.ascontiguousarray(prob["patches"].astype(dtype))
    return dict(name=name, C=C, dtype=dtype, l2=l2, prob=prob, planned=planned, tags=tags)


COMBOS = [(C, dt, l2) for C in (128, 64) for dt in (np.float16, np.float32) for l2 in (True, False)]


def _name(kind, C, dt, l2, n):
    return "%s-C%d-%s-%s-n%d" % (kind, C, np.dtype(dt).name, "l2" if l2 else "raw", n)


def interpolated_references(patches, prob, xy, l2):
    """(i) the reference of every point := the descriptor interpolated at its observation, rounded to fp64: |r|^2 ~ 0."""
    refs = np.empty((len(xy), patches.shape[-1]))
    for o in range(len(xy)):
        k = int(prob["obs_patch"][o])
        _, _, fu, fv, rows, cols = stencil(xy[o], prob["scales"][k], prob["corners"][k])
        T = _texels(patches[k], rows, cols, LD)
        w = np.outer(catmull_rom(fv, LD)[0], catmull_rom(fu, LD)[0]).ravel()
        f = (w[:, None] * T).sum(0)
        if l2:
            f = f / np.sqrt((f * f).sum())
        refs[prob["obs_point"][o]] = f.astype(np.float64)
    return refs


@functools.lru_cache(maxsize=None)
def groups():
    """Every case group: dict(name, C, dtype, l2, prob, planned (n, 2) pixel positions or None, tags)."""
    out = []
    pos = planned_positions()
    uv = np.array([(u, v) for u, v, _ in pos] * len(PATCH_FRAMES))
    tags = [t for _, _, t in pos] * len(PATCH_FRAMES)
    frames = [PATCH_FRAMES[i // len(pos)] for i in range(len(uv))]             # every position in every frame
    for k, (C, dt, l2) in enumerate(COMBOS):                                    # (a)-(e) on smooth unit-norm features (f)
        rng = np.random.default_rng(100 + k)
        prob, xy = placed_problem(uv, frames, smooth_features(rng, len(uv), C).astype(dt), rng=rng,
                                  twins=[(o, o + 1) for o, t in enumerate(tags) if t == "d"])
        out.append(_group(_name("placed", C, dt, l2, len(uv)), C, dt, l2, prob, xy, tags))
    for k, ((C, dt, l2), n) in enumerate(zip(COMBOS, BATCH_SIZES)):            # (g) white noise, every batch size once
        rng = np.random.default_rng(200 + k)
        out.append(_group(_name("noise", C, dt, l2, n), C, dt, l2, shared_problem(rng, n, noise_features(rng, max(1, n // 2), C))))
    rng = np.random.default_rng(300)                                            # (f) smooth, shared patches, the largest batch
    out.append(_group(_name("smooth", 128, np.float16, True, 200), 128, np.float16, True,
                      shared_problem(rng, 200, smooth_features(rng, 100, 128))))
    for k, (C, dt, mag, n) in enumerate([(128, np.float16, 300.0, 65), (64, np.float32, 1e-3, 9), (64, np.float16, 1e-3, 63),
                                         (128, np.float32, 300.0, 7)]):        # (h) x300 / x1e-3, l2 off, reference alike
        rng = np.random.default_rng(400 + k)
        prob = shared_problem(rng, n, (smooth_features(rng, max(1, n // 2), C) * mag).astype(dt))
        prob["refs"] = prob["refs"] * mag
        out.append(_group(_name("x%g" % mag, C, dt, False, n), C, dt, False, prob))
    for k, (C, dt, l2, n) in enumerate([(128, np.float16, True, 64), (64, np.float32, False, 8), (128, np.float32, True, 9),
                                        (64, np.float16, False, 65)]):         # (i) reference = interpolated descriptor
        rng = np.random.default_rng(500 + k)
        uvi = np.column_stack([rng.integers(-1 * 1024, (W + 1) * 1024, n), rng.integers(-1 * 1024, (H + 1) * 1024, n)]) / 1024.0
        patches = (smooth_features if k % 2 == 0 else noise_features)(rng, n, C).astype(dt)
        prob, xy = placed_problem(uvi, PATCH_FRAMES, patches, rng=rng)
        prob["refs"] = interpolated_references(patches, prob, xy, l2)
        out.append(_group(_name("selfref", C, dt, l2, n), C, dt, l2, prob, xy, ["i"] * n))
    for k, (C, l2, n) in enumerate([(128, True, 65), (64, False, 9)]):          # (j) fp16 with +-65504 and subnormals
        rng = np.random.default_rng(600 + k)
        p = noise_features(rng, max(1, n // 2), C).astype(np.float16)
        m = rng.random(p.shape)
        p[m < 0.02] = np.float16(65504.0)
        p[(m >= 0.02) & (m < 0.04)] = np.float16(-65504.0)
        sub = (m >= 0.04) & (m < 0.10)
        p[sub] = (rng.integers(1, 1024, int(sub.sum())) * 2.0 ** -24 * rng.choice([-1.0, 1.0], int(sub.sum()))).astype(np.float16)
        out.append(_group(_name("f16edge", C, np.float16, l2, n), C, np.float16, l2, shared_problem(rng, n, p)))
    for k, (C, l2, n) in enumerate([(128, False, 63), (64, True, 8)]):          # (k) fp32 values fp16 cannot hold
        rng = np.random.default_rng(700 + k)
        p = noise_features(rng, max(1, n // 2), C).astype(np.float32)            # 24-bit significands
        m = rng.random(p.shape)
        p[m < 0.03] *= np.float32(1.0e5)                                         # beyond 65504
        p[(m >= 0.03) & (m < 0.08)] *= np.float32(1.0e-9)                        # below the fp16 subnormals
        assert (p.astype(np.float16).astype(np.float32) != p).mean() > 0.9
        out.append(_group(_name("f32only", C, np.float32, l2, n), C, np.float32, l2, shared_problem(rng, n, p)))
    assert sorted({len(g["prob"]["obs_image"]) for g in out if g["planned"] is None}) == sorted(BATCH_SIZES)
    return out
