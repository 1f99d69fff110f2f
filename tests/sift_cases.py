"""SIFT keypoints and descriptors in numpy float64: the specification that csrc/pxr_sift.hip is held to (a transcription of the
comment above pxr_sift_pyramid in include/pixsfm_hip.h; restated from Lowe's paper and VLFeat's sift.c as remembered -- parity with
VLFeat / COLMAP is unpinned).  Every discrete decision also reports how far it was from flipping (its margin,
in the decision's own units), and rejected candidates stay in the list: the GPU tests need both.

Conventions: pixel-index coordinates (pixel centres at integers), x along columns, y along rows, angles from x towards y."""
import numpy as np

DEFAULTS = dict(first_octave=-1, num_octaves=0, octave_resolution=3, sigma0=1.6, sigma_in=0.5, peak_threshold=-1.0,
                edge_threshold=10.0, max_refine_steps=5, max_num_orientations=2, upright=0, normalization=1, magnif=3.0, clip=0.2)
MAX_OCTAVES, MIN_SIDE = 8, 16


def options(**kw):
    """The options with their defaults; peak_threshold < 0 stands for 0.02 / octave_resolution."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError("unknown SIFT options: %s" % sorted(unknown))
    o = dict(DEFAULTS, **kw)
    if o["peak_threshold"] < 0:
        o["peak_threshold"] = 0.02 / o["octave_resolution"]
    return o


def as_float(image):
    """uint8 -> the float32 quotient u / 255 (what the kernel forms), float32 as it is; returned as float64."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return (image.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    return image.astype(np.float32).astype(np.float64)


def taps(sigma):
    """The weights of a blur by sigma: radius int(4 sigma + 0.5), normalised in float64, rounded to float32."""
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-x * x / (2.0 * sigma * sigma))
    total = 0.0
    for v in w:                                   # in ascending x, as the host code of the library adds them
        total += float(v)
    return (w / total).astype(np.float32).astype(np.float64)


def blur1(a, w, axis):
    """One pass along `axis`, borders replicated; the sum runs over the taps in ascending order from 0."""
    r = len(w) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge")
    acc = np.zeros_like(a)
    n = a.shape[axis]
    for k in range(2 * r + 1):
        acc = acc + w[k] * (p[:, k:k + n] if axis == 1 else p[k:k + n, :])
    return acc


def blur(a, sigma):
    w = taps(sigma)
    return blur1(blur1(a, w, 1), w, 0)          # rows (along x), then columns


def upsample(a):
    """u(2i) = I(i), u(2i + 1) = (I(i) + I(min(i + 1, n - 1))) / 2 along x, then along y."""
    def up(a, axis):
        a = np.moveaxis(a, axis, 0)
        nxt = np.concatenate([a[1:], a[-1:]])
        out = np.empty((2 * a.shape[0],) + a.shape[1:])
        out[0::2], out[1::2] = a, (a + nxt) * 0.5
        return np.moveaxis(out, 0, axis)
    return up(up(a, 1), 0)


def octave_sizes(h, w, opt):
    """[(h_o, w_o)] of the octaves: automatic = while min(h_o, w_o) >= 16, at most 8."""
    if opt["first_octave"] == -1:
        h, w = 2 * h, 2 * w
    sizes = []
    while min(h, w) >= MIN_SIDE and len(sizes) < MAX_OCTAVES:
        sizes.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    if opt["num_octaves"]:
        if opt["num_octaves"] > len(sizes):
            raise ValueError("num_octaves")
        sizes = sizes[:opt["num_octaves"]]
    return sizes


def blur_sigmas(opt):
    """(sigma of the first blur, [sigma of the blur from level s - 1 to s, s = 1 .. S + 2])"""
    S, s0 = opt["octave_resolution"], opt["sigma0"]
    first = np.sqrt(s0 * s0 - (opt["sigma_in"] * 2.0 ** -opt["first_octave"]) ** 2)
    return first, [s0 * np.sqrt(2.0 ** (2.0 * s / S) - 2.0 ** (2.0 * (s - 1) / S)) for s in range(1, S + 3)]


def pyramid(image, opt):
    """[octave: (S + 3, h_o, w_o) float64]; octave index k holds octave first_octave + k."""
    a = as_float(image)
    S = opt["octave_resolution"]
    first, inc = blur_sigmas(opt)
    if opt["first_octave"] == -1:
        a = upsample(a)
    out = []
    for k, (h, w) in enumerate(octave_sizes(image.shape[0], image.shape[1], opt)):
        lv = [blur(a, first) if k == 0 else out[-1][S][0::2, 0::2]]
        assert lv[0].shape == (h, w)
        for s in range(1, S + 3):
            lv.append(blur(lv[-1], inc[s - 1]))
        out.append(np.stack(lv))
    return out


def solve3(A, b):
    """Gaussian elimination with partial pivoting (first largest pivot); None at a zero pivot."""
    A = [[A[i][j] for j in range(3)] + [b[i]] for i in range(3)]
    for c in range(3):
        p = c
        for r in range(c + 1, 3):
            if abs(A[r][c]) > abs(A[p][c]):
                p = r
        if A[p][c] == 0.0:
            return None
        A[c], A[p] = A[p], A[c]
        for r in range(c + 1, 3):
            f = A[r][c] / A[c][c]
            for j in range(c, 4):
                A[r][j] = A[r][j] - f * A[c][j]
    x = [0.0, 0.0, 0.0]
    for c in (2, 1, 0):
        t = A[c][3]
        for j in range(c + 1, 3):
            t = t - A[c][j] * x[j]
        x[c] = t / A[c][c]
    return x


def _refine(D, s, y, x, opt):
    """Refinement of the extremum at (s, y, x) of the DoG stack D.  Returns (accepted, margin, values)."""
    S, peak, e = opt["octave_resolution"], opt["peak_threshold"], opt["edge_threshold"]
    h, w = D.shape[1:]
    margin = np.inf
    mx = my = 0
    for step in range(opt["max_refine_steps"] + 1):
        X, Y = x + mx, y + my
        v = D[s, Y, X]
        g = [0.5 * (D[s, Y, X + 1] - D[s, Y, X - 1]), 0.5 * (D[s, Y + 1, X] - D[s, Y - 1, X]), 0.5 * (D[s + 1, Y, X] - D[s - 1, Y, X])]
        hxx = D[s, Y, X + 1] + D[s, Y, X - 1] - 2.0 * v
        hyy = D[s, Y + 1, X] + D[s, Y - 1, X] - 2.0 * v
        hss = D[s + 1, Y, X] + D[s - 1, Y, X] - 2.0 * v
        hxy = 0.25 * (D[s, Y + 1, X + 1] + D[s, Y - 1, X - 1] - D[s, Y + 1, X - 1] - D[s, Y - 1, X + 1])
        hxs = 0.25 * (D[s + 1, Y, X + 1] + D[s - 1, Y, X - 1] - D[s + 1, Y, X - 1] - D[s - 1, Y, X + 1])
        hys = 0.25 * (D[s + 1, Y + 1, X] + D[s - 1, Y - 1, X] - D[s + 1, Y - 1, X] - D[s - 1, Y + 1, X])
        H = [[hxx, hxy, hxs], [hxy, hyy, hys], [hxs, hys, hss]]
        d = solve3(H, [-g[0], -g[1], -g[2]])
        if d is None:
            return False, 0.0, None
        if step == opt["max_refine_steps"]:
            break
        sx = 1 if (d[0] > 0.6 and X + 1 <= w - 2) else -1 if (d[0] < -0.6 and X - 1 >= 1) else 0
        sy = 1 if (d[1] > 0.6 and Y + 1 <= h - 2) else -1 if (d[1] < -0.6 and Y - 1 >= 1) else 0
        margin = min(margin, abs(abs(d[0]) - 0.6), abs(abs(d[1]) - 0.6))
        if sx == 0 and sy == 0:
            break
        mx, my = mx + sx, my + sy
    val = v + 0.5 * (g[0] * d[0] + g[1] * d[1] + g[2] * d[2])
    det, tr = hxx * hyy - hxy * hxy, hxx + hyy
    bound = (e + 1.0) ** 2 / e
    f = bound * det - tr * tr
    # (passes, distance from flipping) of every test of the acceptance: the value tests in units of the DoG (the determinant
    # through its first-order sensitivity |hxx| + |hyy| + 2 |hxy| to its entries), the offsets, the range of s and the edge ratio
    # tr^2 / det against its bound in their own units
    tests = [(abs(t) < 1.5, abs(abs(t) - 1.5)) for t in d]
    tests += [(s + d[2] >= 0.0, abs(s + d[2])), (s + d[2] <= S + 1, abs(S + 1 - s - d[2])), (abs(val) > peak, abs(abs(val) - peak)),
              (f > 0.0, abs(tr * tr / det - bound) if det != 0.0 else np.inf),
              (det > 0.0, abs(det) / max(abs(hxx) + abs(hyy) + 2.0 * abs(hxy), 1e-300))]
    ok = all(t[0] for t in tests)
    return ok, margin, dict(mx=mx, my=my, d=d, response=abs(val), tests=tests)


def detect(pyr, opt, slack=0.0):
    """Every candidate of the pyramid in ascending (o, s, yi, xi): dicts with the record o, s, xi, yi, `accepted`, `margin` and, where
    the refinement ran, x, y, sigma, response.  A candidate is a DoG sample at s in 1 .. S, one pixel inside the border, with
    |D| > 0.8 peak_threshold - slack that is above (or below) all 26 neighbours by more than -slack; with slack = 0 these are the
    candidates of the specification (`strict`), with slack > 0 also the samples that a perturbation of that size could turn into one."""
    S, peak = opt["octave_resolution"], opt["peak_threshold"]
    out = []
    for k, G in enumerate(pyr):
        o = opt["first_octave"] + k
        D = G[1:] - G[:-1]
        h, w = D.shape[1:]
        if h < 3 or w < 3:
            continue
        c = D[1:S + 1, 1:h - 1, 1:w - 1]
        hi = np.full(c.shape, -np.inf)
        lo = np.full(c.shape, np.inf)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if ds == dy == dx == 0:
                        continue
                    n = D[1 + ds:S + 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    hi, lo = np.maximum(hi, n), np.minimum(lo, n)
        gap = np.maximum(c - hi, lo - c)                    # > 0: a strict extremum
        strong = np.abs(c) - 0.8 * peak
        for s, y, x in np.argwhere((gap > -slack) & (strong > -slack)):
            tests = [(gap[s, y, x] > 0, abs(gap[s, y, x])), (strong[s, y, x] > 0, abs(strong[s, y, x]))]
            s, y, x = int(s) + 1, int(y) + 1, int(x) + 1
            cand = dict(o=o, s=s, xi=x, yi=y, accepted=False, strict=bool(tests[0][0] and tests[1][0]))
            ok, path, r = _refine(D, s, y, x, opt)
            tests += r["tests"] if r is not None else [(False, np.inf)]
            # margin: the smallest distance of any decision from flipping; reject_gap: how far a rejected candidate is from
            # acceptance -- the largest distance among its failed tests, or 0 where a decision of the refinement's path is that close
            cand["path_margin"] = path
            cand["margin"] = min([path] + [t[1] for t in tests])
            cand["reject_gap"] = max([0.0] + [t[1] for t in tests if not t[0]])
            if r is not None:
                d = r["d"]
                cand.update(x=(x + r["mx"] + d[0]) * 2.0 ** o, y=(y + r["my"] + d[1]) * 2.0 ** o, s_ref=s + d[2],
                            sigma=opt["sigma0"] * 2.0 ** (o + (s + d[2]) / S), response=r["response"])
            cand["accepted"] = all(t[0] for t in tests)
            out.append(cand)
    return out


def _gradients(L, px, py):
    gx = 0.5 * (L[py, px + 1] - L[py, px - 1])
    gy = 0.5 * (L[py + 1, px] - L[py - 1, px])
    return np.sqrt(gx * gx + gy * gy), np.mod(np.arctan2(gy, gx), 2.0 * np.pi)


def _window(L, xo, yo, R):
    """The integer samples within R of (round(xo), round(yo)) that have all four neighbours inside the level."""
    h, w = L.shape
    xi, yi = int(np.floor(xo + 0.5)), int(np.floor(yo + 0.5))
    ys, xs = np.mgrid[yi - R:yi + R + 1, xi - R:xi + R + 1]
    ys, xs = ys.ravel(), xs.ravel()                       # rows first: the kernel's sample order
    keep = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)
    return xs[keep], ys[keep]


def orientation_histogram(L, xo, yo, sigma_oct):
    """The smoothed 36-bin histogram."""
    sw = 1.5 * sigma_oct
    R = int(np.floor(3.0 * sw))
    xs, ys = _window(L, xo, yo, R)
    dx, dy = xs - xo, ys - yo
    d2 = dx * dx + dy * dy
    keep = d2 < R * R + 0.5
    xs, ys, d2 = xs[keep], ys[keep], d2[keep]
    mag, ang = _gradients(L, xs, ys)
    v = mag * np.exp(-d2 / (2.0 * sw * sw))
    fbin = 36.0 * ang / (2.0 * np.pi) - 0.5
    d = fbin[:, None] - np.arange(36.0)[None, :]
    d = d - 36.0 * np.floor(d / 36.0 + 0.5)                # circular difference in [-18, 18)
    hist = (v[:, None] * np.maximum(0.0, 1.0 - np.abs(d))).sum(0)
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / 3.0
    return hist


def orientations(L, xo, yo, sigma_oct, opt):
    """([theta by rank], margin): the peaks of the histogram by (height descending, bin ascending), at most max_num_orientations.
    The margin is the smallest gap, in units of the histogram (gradient magnitudes times window weights), of any bin's three
    comparisons and of the order of the ranks."""
    if opt["upright"]:
        return [0.0], np.inf
    hist = orientation_histogram(L, xo, yo, sigma_oct)
    top = hist.max()
    peaks, margin = [], np.inf
    for i in range(36):
        h0, hm, hp = hist[i], hist[(i + 35) % 36], hist[(i + 1) % 36]
        gaps = [h0 - hm, h0 - hp, h0 - 0.8 * top]
        if h0 > hm and h0 > hp and h0 >= 0.8 * top:
            margin = min(margin, min(gaps))
            di = -0.5 * (hp - hm) / (hp + hm - 2.0 * h0)
            peaks.append((h0, i, 2.0 * np.pi * (i + di + 0.5) / 36.0))
        else:
            margin = min(margin, max(-g for g in gaps if not g > 0) if any(not g > 0 for g in gaps) else 0.0)
    peaks.sort(key=lambda p: (-p[0], p[1]))
    K = opt["max_num_orientations"]
    for a, b in zip(peaks[:K], peaks[1:K + 1]):
        margin = min(margin, a[0] - b[0])                   # the order of the ranks, and who falls off the end
    return [p[2] for p in peaks[:K]], margin


def level_of_sigma(sigma, opt, n_octaves):
    """(octave index k, level, sigma in the octave's pixels) that describe() uses for a keypoint of scale sigma; None outside."""
    S = opt["octave_resolution"]
    if n_octaves == 0:
        return None
    t = S * np.log2(sigma / opt["sigma0"])
    first = opt["first_octave"]
    o = int(min(max(np.floor((t - 0.5) / S), first), first + n_octaves - 1))      # clamped to the pyramid's octaves
    k = o - first
    level = int(min(max(np.floor(t - o * S + 0.5), -1), S + 3))
    if level < 0 or level > S + 2:
        return None
    return k, level, sigma * 2.0 ** -o


def descriptor(L, xo, yo, sigma_oct, theta, opt):
    """The 128 values (by, bx, bo) of one feature on level L, as float64 before the cast to float32; (desc, valid, clamped_norm)."""
    sbp = opt["magnif"] * sigma_oct
    W = int(np.floor(np.sqrt(2.0) * sbp * 2.5 + 0.5))
    xs, ys = _window(L, xo, yo, W)
    dx, dy = xs - xo, ys - yo
    mag, ang = _gradients(L, xs, ys)
    ct, st = np.cos(theta), np.sin(theta)
    nx, ny = (ct * dx + st * dy) / sbp, (-st * dx + ct * dy) / sbp
    ft = 8.0 * np.mod(ang - theta, 2.0 * np.pi) / (2.0 * np.pi)
    v = mag * np.exp(-(nx * nx + ny * ny) / 8.0)            # sigma of the window: 2 bins
    fx, fy = nx + 1.5, ny + 1.5                               # bin b of 0 .. 3 has its centre at b
    wx = np.maximum(0.0, 1.0 - np.abs(fx[:, None] - np.arange(4.0)))
    wy = np.maximum(0.0, 1.0 - np.abs(fy[:, None] - np.arange(4.0)))
    dt = ft[:, None] - np.arange(8.0)
    dt = dt - 8.0 * np.floor(dt / 8.0 + 0.5)
    wt = np.maximum(0.0, 1.0 - np.abs(dt))
    hist = np.einsum("n,ny,nx,nt->yxt", v, wy, wx, wt).ravel()
    norm = np.sqrt((hist * hist).sum())
    if not norm > 0.0:
        return np.zeros(128), False, 0.0
    hist = np.minimum(hist / norm, opt["clip"])
    norm2 = np.sqrt((hist * hist).sum())
    hist = hist / norm2
    if opt["normalization"] == 1:
        hist = np.sqrt(hist / hist.sum())
    return hist, True, norm2


def describe(pyr, opt, keypoints):
    """(n, 4) x, y, sigma, theta -> ((n, 128) float64, (n,) bool): zeros and False for a keypoint that is not finite, has
    sigma <= 0 or a scale outside the pyramid."""
    kp = np.asarray(keypoints, dtype=np.float64).reshape(-1, 4)
    out, valid = np.zeros((len(kp), 128)), np.zeros(len(kp), dtype=bool)
    for i, (x, y, sigma, theta) in enumerate(kp):
        if not np.isfinite([x, y, sigma, theta]).all() or sigma <= 0:
            continue
        lv = level_of_sigma(sigma, opt, len(pyr))
        if lv is None:
            continue
        k, level, sigma_oct = lv
        scale = 2.0 ** -(opt["first_octave"] + k)
        out[i], valid[i], _ = descriptor(pyr[k][level], x * scale, y * scale, sigma_oct, theta, opt)
    return out, valid


def features(pyr, opt, candidates=None):
    """The accepted keypoints with their orientations, in the order of the output: dict of keypoints (n, 4) x, y, sigma, theta,
    record (n, 4) o, s, xi, yi, response (n,), orientation_margin (n,)."""
    S = opt["octave_resolution"]
    cands = detect(pyr, opt) if candidates is None else candidates
    kps, rec, resp, om = [], [], [], []
    for c in cands:
        if not c["accepted"]:
            continue
        k = c["o"] - opt["first_octave"]
        level = min(max(int(np.floor(c["s_ref"] + 0.5)), 0), S + 2)
        scale = 2.0 ** -c["o"]
        thetas, m = orientations(pyr[k][level], c["x"] * scale, c["y"] * scale, c["sigma"] * scale, opt)
        for th in thetas:
            kps.append([c["x"], c["y"], c["sigma"], th])
            rec.append([c["o"], c["s"], c["xi"], c["yi"]])
            resp.append(c["response"])
            om.append(m)
    return dict(keypoints=np.array(kps, dtype=np.float64).reshape(-1, 4), record=np.array(rec, dtype=np.int32).reshape(-1, 4),
                response=np.array(resp, dtype=np.float64), orientation_margin=np.array(om, dtype=np.float64))


def extract(image, **kw):
    """Image -> (features dict with descriptors (n, 128) and valid, pyramid, candidates)."""
    opt = options(**kw)
    pyr = pyramid(image, opt)
    cands = detect(pyr, opt)
    f = features(pyr, opt, cands)
    f["descriptors"], f["valid"] = describe(pyr, opt, f["keypoints"])
    return f, pyr, cands


def pass_bound(image, opt):
    """The derived bound on |float32 pyramid - this reference| per (octave index, level): every pass adds (taps + 1) 2^-24 times the
    value range; the upsampling counts as two passes of two taps."""
    a = as_float(image)
    rng = float(a.max() - a.min()) if a.size else 0.0
    u = 2.0 ** -24 * max(rng, np.abs(a).max() if a.size else 0.0)
    S = opt["octave_resolution"]
    first, inc = blur_sigmas(opt)
    chain = 2 * 3 * u if opt["first_octave"] == -1 else 0.0
    out = []
    for k in range(len(octave_sizes(a.shape[0], a.shape[1], opt))):
        row = [chain + 2 * (len(taps(first)) + 1) * u if k == 0 else out[-1][S]]
        for s in range(1, S + 3):
            row.append(row[-1] + 2 * (len(taps(inc[s - 1])) + 1) * u)
        out.append(row)
    return out


# ---- images -----------------------------------------------------------------------------------------------------------------
def blob_image(h, w, blobs, background=0.5):
    """float32 image of Gaussian blobs (cx, cy, std, amplitude) on a flat background."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), background)
    for cx, cy, std, amp in blobs:
        a += amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2.0 * std * std))
    return a.astype(np.float32)


def blob_grid(n, std=3.0, pitch=28, seed=0):
    """An image of n isolated blobs on a grid (sub-pixel centres, both signs) and the blob list."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n)))
    rows = (n + cols - 1) // cols
    blobs = []
    for i in range(n):
        cx = pitch * (i % cols) + pitch / 2.0 + rng.uniform(-0.3, 0.3)
        cy = pitch * (i // cols) + pitch / 2.0 + rng.uniform(-0.3, 0.3)
        blobs.append((cx, cy, std, 0.4 if i % 2 == 0 else -0.4))
    return blob_image(rows * pitch, cols * pitch, blobs), blobs


def oriented_scene(h, w, seed, pitch=26, dtype=np.float32, amp=0.45):
    """An image of strong, well-separated structures with a clear orientation each: on a jittered grid a Gaussian blob (std 2.4 ..
    3.6, both signs) cut by a smooth step through its centre at a random angle, on a flat background.  float32, or uint8 by
    rounding."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 0.5)
    ny, nx = max(h // pitch, 1), max(w // pitch, 1)
    for gy in range(ny):
        for gx in range(nx):
            cx = (gx + 0.5) * w / nx + rng.uniform(-0.3, 0.3)
            cy = (gy + 0.5) * h / ny + rng.uniform(-0.3, 0.3)
            std, ang, sign = rng.uniform(2.4, 3.6), rng.uniform(0.0, 2.0 * np.pi), 1.0 if (gx + gy) % 2 else -1.0
            u = (xs - cx) * np.cos(ang) + (ys - cy) * np.sin(ang)
            a += sign * amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2.0 * std * std)) * 0.5 * (1.0 + np.tanh(u / 0.8))
    a = a.astype(np.float32)
    return a if dtype == np.float32 else np.round(255.0 * np.clip(a, 0.0, 1.0)).astype(np.uint8)


def perturbed(pyr, bound, seed):
    """The pyramid with every sample moved by + or - the bound of its level, signs at random: what the float32 kernels may return."""
    rng = np.random.default_rng(seed)
    return [G + np.array(b)[:, None, None] * rng.choice([-1.0, 1.0], size=G.shape) for G, b in zip(pyr, bound)]


def sensitivity(image, opt, seeds=(0, 1)):
    """How far the outputs of the reference move when its pyramid is perturbed by the derived bound (the figures written into
    tests/test_sift_gpu.py): the largest change of x / y, sigma (relative), response, theta and of a descriptor entry, over the
    keypoints both runs accept whose margins exceed eps = 8 bound.  The descriptors are those of the unperturbed keypoints on
    both pyramids."""
    pyr = pyramid(image, opt)
    bound = pass_bound(image, opt)
    eps = 8.0 * max(max(b) for b in bound)
    base = features(pyr, opt)
    d0, _ = describe(pyr, opt, base["keypoints"])
    cands = {(c["o"], c["s"], c["xi"], c["yi"]): c for c in detect(pyr, opt)}
    out = dict(xy=0.0, sigma=0.0, response=0.0, theta=0.0, desc=0.0)
    for seed in seeds:
        p = perturbed(pyr, bound, seed)
        f = features(p, opt)
        d1, _ = describe(p, opt, base["keypoints"])
        out["desc"] = max(out["desc"], float(np.abs(d1 - d0).max()) if len(d0) else 0.0)
        rows = {}
        for i, r in enumerate(f["record"]):
            rows.setdefault(tuple(r), []).append(i)
        seen = {}
        for i, r in enumerate(base["record"]):
            c = cands[tuple(r)]
            j = rows.get(tuple(r))
            rank = seen.get(tuple(r), 0)
            seen[tuple(r)] = rank + 1
            if j is None or c["margin"] <= eps or base["orientation_margin"][i] <= eps or rank >= len(j):
                continue
            a, b = base["keypoints"][i], f["keypoints"][j[rank]]
            out["xy"] = max(out["xy"], abs(a[0] - b[0]), abs(a[1] - b[1]))
            out["sigma"] = max(out["sigma"], abs(a[2] / b[2] - 1.0))
            dth = abs(a[3] - b[3])
            out["theta"] = max(out["theta"], min(dth, 2.0 * np.pi - dth))
            out["response"] = max(out["response"], abs(base["response"][i] - f["response"][j[rank]]))
    return out


def textured_image(h, w, seed, smooth=1.5):
    """uint8 image of smoothed noise with full contrast: many extrema at several scales."""
    rng = np.random.default_rng(seed)
    a = blur(rng.standard_normal((h, w)), smooth) + 0.5 * blur(rng.standard_normal((h, w)), 3.0 * smooth)
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(255.0 * a).astype(np.uint8)
