"""The numpy reference of SIFT (tests/sift_cases.py) pinned on the CPU: against scipy's Gaussian filter, on blobs whose position
and scale are known, under a quarter turn of the image, and on the properties of its descriptors."""
import numpy as np
import pytest

import sift_cases as sc


@pytest.fixture(scope="module")
def texture():
    return sc.textured_image(97, 131, 1)


@pytest.mark.parametrize("first_octave", [-1, 0])
def test_levels_against_scipy(texture, first_octave):
    """One pass of the reference is scipy's gaussian_filter1d(truncate=4, mode="nearest") with float32-rounded weights: every level
    is scipy's blur of the level before (measured 2.3e-8, the rounding of the weights; held to twice that).  Against ONE direct
    blur of the image by sqrt(sigma_abs^2 - sigma_in^2) the incremental, truncated chain differs.  Farther than 4 sigma + 2 from the
    border: measured 1.04e-5 for first_octave 0 (the truncation of every increment at 4 sigma), and 5.6e-3 for first_octave -1,
    where the doubling by linear interpolation is not the Gaussian of sigma_in that the first blur assumes; both held to twice
    the measured value.  At the border replication does not compose (an increment replicates the blurred edge, the direct blur
    the raw one): measured 0.057 and 0.061, held to twice that."""
    from scipy.ndimage import gaussian_filter
    opt = sc.options(first_octave=first_octave)
    S = opt["octave_resolution"]
    a = sc.as_float(texture)
    pyr = sc.pyramid(texture, opt)
    _, inc = sc.blur_sigmas(opt)
    assert [p.shape[1:] for p in pyr] == sc.octave_sizes(97, 131, opt)
    inner = border = step = 0.0
    for k, G in enumerate(pyr):
        o = first_octave + k
        for s in range(S + 3):
            if s > 0:
                step = max(step, np.abs(gaussian_filter(G[s - 1], inc[s - 1], truncate=4, mode="nearest") - G[s]).max())
            if o < 0:
                continue
            sigma = opt["sigma0"] * 2.0 ** (o + s / S)
            ref = gaussian_filter(a, np.sqrt(sigma * sigma - opt["sigma_in"] ** 2), truncate=4, mode="nearest")[::2 ** o, ::2 ** o]
            d = np.abs(ref - G[s])
            m = int(np.ceil(4.0 * sigma / 2 ** o)) + 2
            border = max(border, d.max())
            if min(d.shape) > 2 * m + 4:
                inner = max(inner, d[m:-m, m:-m].max())
    print("first_octave %d: step %.3g inner %.3g border %.3g" % (first_octave, step, inner, border))
    assert step <= 2 * 2.4e-8
    assert 0.0 < inner <= 2 * (5.6e-3 if first_octave == -1 else 1.04e-5)
    assert border <= 2 * (0.0613 if first_octave == -1 else 0.0569)


def test_upsampling_halves_coordinates_exactly():
    a = np.arange(12.0).reshape(3, 4)
    u = sc.upsample(a)
    assert u.shape == (6, 8) and np.array_equal(u[0::2, 0::2], a)
    assert np.array_equal(u[0, 1::2], [0.5, 1.5, 2.5, 3.0]) and np.array_equal(u[1::2, 0], [2.0, 6.0, 8.0])


@pytest.mark.parametrize("first_octave", [-1, 0])
def test_blobs_are_found_at_their_centre_and_scale(first_octave):
    """Isolated Gaussian blobs of std 2.5 .. 6 px, sub-pixel centres, both signs: exactly one keypoint per blob.  Position: the
    reference achieves 0.033 px here, held to 0.07.  Scale: the scale-normalised LoG of a Gaussian blob peaks at the blob's std,
    and the difference of Gaussians between sigma and 2^(1/S) sigma stands for the Laplacian at a scale between the two while the
    keypoint is labelled with the lower one: measured sigma / std in [0.870, 0.890] for S = 3, i.e. |sigma / std - 1| <= 0.13,
    held to 0.26."""
    rng = np.random.default_rng(2)
    stds = [2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0]
    blobs = [(40 + 80 * (i % 4) + rng.uniform(-0.5, 0.5), 40 + 80 * (i // 4) + rng.uniform(-0.5, 0.5), sd, 0.4 if i % 2 else -0.4)
             for i, sd in enumerate(stds)]
    image = sc.blob_image(160, 320, blobs)
    opt = sc.options(first_octave=first_octave)
    found = [c for c in sc.detect(sc.pyramid(image, opt), opt) if c["accepted"]]
    assert len(found) == len(blobs)
    taken = set()
    for c in found:
        j = int(np.argmin([(c["x"] - b[0]) ** 2 + (c["y"] - b[1]) ** 2 for b in blobs]))
        taken.add(j)
        assert np.hypot(c["x"] - blobs[j][0], c["y"] - blobs[j][1]) <= 0.07
        assert abs(c["sigma"] / blobs[j][2] - 1.0) <= 0.26
    assert len(taken) == len(blobs)


@pytest.mark.parametrize("kw", [dict(first_octave=0), dict(first_octave=0, normalization=0, max_num_orientations=4, octave_resolution=2),
                                dict(first_octave=0, upright=1)], ids=["defaults", "L2_S2_four_orientations", "upright"])
def test_quarter_turn(kw):
    """np.rot90 of the image turns the keypoints, shifts theta by a quarter turn and permutes the descriptor's channels, to 1e-9:
    every index convention, checked independently of how it was written.  rot90 (counter-clockwise on the screen) maps the pixel
    (x, y) of an h x w image to (y, w - 1 - x); a direction (dx, dy) goes to (dy, -dx), so the angle from x towards y drops by
    pi / 2.  The window is symmetric under the turn, and so is the blur (rows then columns with the same taps), up to the order of
    its two passes -- a rounding, not a convention.  The turn reverses the axis of length w, and an octave keeps the EVEN indices of
    the one before, which is symmetric under reversal only for an odd length: w = 61 -> 31 covers both octaves of this image.  The
    doubling of first_octave = -1 puts pixel i at 2 i of 2 w pixels, which no reversal maps onto itself, so that octave has no
    such symmetry; its coordinates are pinned by the blobs above."""
    image = sc.textured_image(48, 61, 7)
    h, w = image.shape
    f0, _, _ = sc.extract(image, **kw)
    f1, _, _ = sc.extract(np.ascontiguousarray(np.rot90(image)), **kw)
    n = len(f0["keypoints"])
    assert n >= 10 and len(f1["keypoints"]) == n
    k0 = f0["keypoints"]
    turned = np.column_stack([k0[:, 1], (w - 1) - k0[:, 0], k0[:, 2], np.mod(k0[:, 3] - np.pi / 2, 2 * np.pi)])
    used = set()
    for i in range(n):
        dth = np.abs(f1["keypoints"][:, 3] - turned[i, 3])
        dth = np.minimum(dth, 2 * np.pi - dth) if not kw.get("upright") else 0.0 * dth
        d = np.maximum(np.abs(f1["keypoints"][:, :3] - turned[i, :3]).max(1), dth)
        j = int(np.argmin(d))
        assert d[j] <= 1e-9 and j not in used
        used.add(j)
        if kw.get("upright"):
            # theta = 0 in both images: the descriptor's frame did not turn with the image, so only position and scale are compared
            continue
        # the frame turned with the image, so the descriptor is the same vector, channel for channel
        assert np.abs(f1["descriptors"][j] - f0["descriptors"][i]).max() <= 1e-9


def test_upright_descriptor_channels_permute_under_a_quarter_turn():
    """With theta fixed at 0 the frame stays with the axes, and a quarter turn of the image permutes the channels: the bin
    (by, bx, bo) of the original is the bin (3 - bx, by, bo - 2 mod 8) of the turned image."""
    image = sc.textured_image(48, 61, 7)
    h, w = image.shape
    kw = dict(first_octave=0, upright=1)
    f0, _, _ = sc.extract(image, **kw)
    f1, _, _ = sc.extract(np.ascontiguousarray(np.rot90(image)), **kw)
    k0 = f0["keypoints"]
    turned = np.column_stack([k0[:, 1], (w - 1) - k0[:, 0], k0[:, 2]])
    assert len(k0) >= 10
    for i in range(len(k0)):
        j = int(np.argmin(np.abs(f1["keypoints"][:, :3] - turned[i]).max(1)))
        d0 = f0["descriptors"][i].reshape(4, 4, 8)
        d1 = f1["descriptors"][j].reshape(4, 4, 8)
        perm = np.empty_like(d0)
        for by in range(4):
            for bx in range(4):
                for bo in range(8):
                    perm[3 - bx, by, (bo - 2) % 8] = d0[by, bx, bo]
        assert np.abs(d1 - perm).max() <= 1e-9


@pytest.mark.parametrize("normalization", [0, 1])
def test_descriptor_properties(texture, normalization):
    """Unit L2 norm; no value above what the clamp allows: clip / |clamped| after the second L2 (L2), and the square root of that
    value's share of the L1 norm (L1_ROOT) -- both below 1 / sqrt(number of clamped entries) <= 1, and checked exactly here from
    the norm the reference reports."""
    opt = sc.options(normalization=normalization)
    pyr = sc.pyramid(texture, opt)
    f = sc.features(pyr, opt)
    desc, valid = sc.describe(pyr, opt, f["keypoints"])
    assert valid.all() and len(desc) > 100
    assert np.abs(np.linalg.norm(desc, axis=1) - 1.0).max() <= 1e-12
    assert (desc >= 0).all()
    S = opt["octave_resolution"]
    for kp, d in list(zip(f["keypoints"], desc))[::7]:
        k, level, sigma_oct = sc.level_of_sigma(kp[2], opt, len(pyr))
        scale = 2.0 ** -(opt["first_octave"] + k)
        _, _, norm2 = sc.descriptor(pyr[k][level], kp[0] * scale, kp[1] * scale, sigma_oct, kp[3], sc.options(normalization=0))
        top = opt["clip"] / norm2
        if normalization == 0:
            assert d.max() <= top + 1e-12
        else:
            l2 = sc.descriptor(pyr[k][level], kp[0] * scale, kp[1] * scale, sigma_oct, kp[3], sc.options(normalization=0))[0]
            assert d.max() <= np.sqrt(top / l2.sum()) + 1e-12
    # the cases describe() refuses
    bad = np.array([[np.nan, 3, 2, 0], [3, 3, -1, 0], [3, 3, 1e-3, 0], [3, 3, 1e6, 0], [-500, 20, 2, 0]])
    d, v = sc.describe(pyr, opt, bad)
    assert not v.any() and (d == 0).all()


def test_candidates_margins_and_order(texture):
    opt = sc.options()
    pyr = sc.pyramid(texture, opt)
    cands = sc.detect(pyr, opt)
    keys = [(c["o"], c["s"], c["yi"], c["xi"]) for c in cands]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert any(c["accepted"] for c in cands) and any(not c["accepted"] for c in cands)
    assert all(c["margin"] >= 0 and c["accepted"] == (c["reject_gap"] == 0) for c in cands)
    wide = sc.detect(pyr, opt, slack=1e-4)
    assert len(wide) > len(cands) and {(c["o"], c["s"], c["yi"], c["xi"]) for c in cands} <= {(c["o"], c["s"], c["yi"], c["xi"]) for c in wide}
    assert [c["accepted"] for c in wide if (c["o"], c["s"], c["yi"], c["xi"]) in set(keys)] == [c["accepted"] for c in cands]
