"""One SHA-256 per case over every output of the batched geometry stages -- absolute pose, two-view geometry (estimating, and
with a pose prior), triangulation, descriptor matching, homography and fundamental-matrix estimation -- timings excluded.

A refactor of pxr_abspose.hip, pxr_twoview.hip, pxr_triangulate.hip, pxr_match.hip, pxr_homography.hip, pxr_fundamental.hip or of
what they share (pxr_robust.h, pxr_batch.h, pxr_pairs.h) must leave every line of this output unchanged: run it
before and after on the same machine and compare.  Only the
public engine API is used, and the seeded generators the tests use (tests/*_cases.py, the repository's own oracle for the
camera models).

  python tools/geometry_fingerprint.py            # prints "<case> <sha256>" per line
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pixel-perfect-sfm_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def digest(device_arrays):
    h = hashlib.sha256()
    for a in device_arrays:
        h.update(np.ascontiguousarray(a.download()).tobytes())
    return h.hexdigest()


def abspose(ctx, batch):
    from pixsfm_amd.engine import AbsolutePoseProblem
    return digest(AbsolutePoseProblem(ctx, batch).estimate())


def twoview(ctx, batch):
    from pixsfm_amd.engine import TwoViewProblem
    return digest(TwoViewProblem(ctx, batch).estimate())


def homography(ctx, batch):
    from pixsfm_amd.engine import HomographyProblem
    return digest(HomographyProblem(ctx, batch).estimate())


def fundamental(ctx, batch):
    from pixsfm_amd.engine import FundamentalProblem
    return digest(FundamentalProblem(ctx, batch).estimate())


def triangulation(ctx, scene):
    from pixsfm_amd.engine import TriangulationProblem
    return digest(TriangulationProblem(ctx, scene).triangulate())


def matching(ctx, descriptors, pairs, options):
    from pixsfm_amd.engine import MatchProblem
    return digest(MatchProblem(ctx, descriptors, pairs).run(**options))


def cases(ctx):
    import abspose_cases as ac
    import matching_cases as mc
    import triangulation_cases as tc
    import twoview_cases as tv
    queries, pairs = ac.boundary_inputs(), tv.boundary_inputs()
    yield "abspose_boundaries", lambda: abspose(ctx, queries)
    yield "twoview_boundaries", lambda: twoview(ctx, pairs)
    yield "twoview_boundaries_prior", lambda: twoview(ctx, dict(pairs, prior_qvec=pairs["gt_qvec"], prior_tvec=3.0 * pairs["gt_tvec"]))
    # track lengths around the 16-lane group, the LDS staging limit and the hypothesis cap (tests/test_triangulation_gpu.py)
    lengths = np.repeat((0, 1, 2, 3, 15, 16, 17, 23, 24, 33, 64, 65, 97), 23)
    lengths = lengths[np.random.default_rng(1).permutation(len(lengths))]
    yield "triangulation_boundaries", lambda: triangulation(ctx, tc.make_scene(lengths, n_cams=96, models=(2,), seed=3))
    yield "triangulation_statuses", lambda: triangulation(ctx, tc.status_scene())
    for shape in mc.GPU_SHAPES:
        A, B = mc.pair_case(*shape, seed=100 + mc.GPU_SHAPES.index(shape))
        for name, options in mc.OPTION_SETS.items():
            yield "matching_%s_%s" % ("x".join(map(str, shape)), name), lambda A=A, B=B, o=options: matching(ctx, [A, B], [(0, 1)], o)
    descs, image_pairs = mc.batch_case()
    for name in ("NN-ratio", "NN-ratio-one-way"):
        yield "matching_batch_" + name, lambda o=mc.OPTION_SETS[name]: matching(ctx, descs, image_pairs, o)
    (q11, _, _), (p11, _, _), models = ac.eleven_models_queries(), tv.eleven_models_pairs(), sorted(tc.MODEL_PARAMS)
    yield "abspose_eleven_models", lambda: abspose(ctx, q11)
    yield "twoview_eleven_models", lambda: twoview(ctx, p11)
    scene = tc.make_scene(np.random.default_rng(2).integers(2, 12, 4 * len(models)), n_cams=2 * len(models), models=tuple(models), seed=4, arc=9)
    yield "triangulation_eleven_models", lambda: triangulation(ctx, scene)
    import homography_cases as hc
    planes = hc.boundary_inputs()
    yield "homography_boundaries", lambda: homography(ctx, planes)
    yield "homography_eleven_models", lambda: homography(ctx, hc.eleven_models_pairs()[0])
    import fundamental_cases as fc
    uncalibrated = fc.boundary_inputs()
    yield "fundamental_boundaries", lambda: fundamental(ctx, uncalibrated)
    yield "fundamental_eleven_models", lambda: fundamental(ctx, fc.eleven_models_pairs()[0])


if __name__ == "__main__":
    from pixsfm_amd.engine import Context
    context = Context(0)
    try:
        for name, run in cases(context):
            print("%-44s %s" % (name, run()), flush=True)
    finally:
        context.close()
