"""The cases of tests/test_sift_gpu.py: images, options, and what the reference alone says about them (computed once, shared)."""
import functools

import numpy as np

import sift_cases as sc

# name -> (image maker, options, holds the margin condition).  The images and seeds were chosen on the CPU so that at most 5 % of the
# reference's keypoints (and of its features' orientations) have a margin <= eps; "texture" is an additional stress case of many
# weak keypoints for which no image can meet that condition (the gap of a DoG sample to its neighbours is of the order of eps).
CASES = {
    "17x23_smaller_than_a_tile": (lambda: sc.oriented_scene(17, 23, 0), dict(), True),
    "65x63_u8": (lambda: sc.oriented_scene(65, 63, 1, dtype=np.uint8), dict(), True),
    "64x64_octave0": (lambda: sc.oriented_scene(64, 64, 0), dict(first_octave=0), True),
    "97x131_three_octaves": (lambda: sc.oriented_scene(97, 131, 13), dict(first_octave=0), True),
    "80x90_S2_L2": (lambda: sc.oriented_scene(80, 90, 0), dict(first_octave=0, octave_resolution=2, normalization=0), True),
    "80x90_S4_upright": (lambda: sc.oriented_scene(80, 90, 6), dict(first_octave=0, octave_resolution=4, upright=1), True),
    "70x75_u8_four_orientations": (lambda: sc.oriented_scene(70, 75, 4, dtype=np.uint8), dict(first_octave=0, max_num_orientations=4), True),
    "grid_1": (lambda: sc.blob_grid(1, std=2.2, pitch=24)[0], dict(first_octave=0, upright=1), True),
    "grid_63": (lambda: sc.blob_grid(63, std=2.2, pitch=24)[0], dict(first_octave=0, upright=1), True),
    "grid_64": (lambda: sc.blob_grid(64, std=2.2, pitch=24)[0], dict(first_octave=0, upright=1), True),
    "grid_65": (lambda: sc.blob_grid(65, std=2.2, pitch=24)[0], dict(first_octave=0, upright=1), True),
    "grid_257": (lambda: sc.blob_grid(257, std=2.2, pitch=24)[0], dict(first_octave=0, upright=1), True),
    "view_320": (lambda: real_view(), dict(first_octave=0, num_octaves=1, peak_threshold=0.06), True),
    "texture_97x131_octave-1": (lambda: sc.textured_image(97, 131, 1), dict(), False),
}
GRID_COUNTS = {"grid_1": 1, "grid_63": 63, "grid_64": 64, "grid_65": 65, "grid_257": 257}


def real_view():
    """One 320 x 320 view of a golden tile (real_scene.render_view), grey, uint8."""
    import real_scene as rs
    Rs, ts = rs.cameras(2, 4)
    return np.round(rs.render_view(rs.load_tile(0), Rs[1], ts[1]).mean(0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(image, opt, kw, pyr, bound, eps, cands (with slack eps), feats)"""
    make, kw, _ = CASES[name]
    image = make()
    opt = sc.options(**kw)
    pyr = sc.pyramid(image, opt)
    bound = sc.pass_bound(image, opt)
    eps = 8.0 * max([max(b) for b in bound] + [0.0])
    cands = sc.detect(pyr, opt, slack=eps)
    strict = [c for c in cands if c["strict"]]
    return dict(image=image, opt=opt, kw=kw, pyr=pyr, bound=bound, eps=eps, cands=cands, feats=sc.features(pyr, opt, strict))
