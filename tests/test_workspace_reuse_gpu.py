"""GPU: one context's grow-only workspace handed from driver to driver (csrc/pxr_batch.h Workspace, csrc/pxr_internal.h
grow_block).  Every per-stage test runs its driver on a workspace that the same driver sized; here five drivers with five layouts
follow each other on ONE context -- a small layout, larger ones that must grow the block, one (the KA solve's) that may release the
context's caches to grow, one that commits into a block left larger by its predecessor and must not grow, and the first again on
the block the others left -- and every output must equal, bit for bit, what the same call returns on a fresh context.  A driver
that kept a pointer into a block that was freed, read an array it had not written, or laid two arrays over each other would show
as a difference (or as a fault)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import global_mapping_cases as gc
import triangulation_cases as tc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_graph_gpu import _flat_random_graph  # noqa: E402

pytestmark = pytest.mark.gpu


def _triangulation(ctx):
    """Three tracks (2, 5 and 17 observations)."""
    from pixsfm_amd.engine import TriangulationProblem
    scene = tc.make_scene(np.array([2, 5, 17]), n_cams=24, models=(2,), seed=3)
    out = TriangulationProblem(ctx, scene).triangulate()
    return dict(zip(("xyz", "status", "n_inliers", "obs_inlier", "obs_err"), (a.download() for a in out)))


def _graph(ctx):
    """Labels, scores and roots of a match graph on 40 nodes."""
    from pixsfm_amd import _lib
    node_image, src, dst, sim = _flat_random_graph(np.random.default_rng(4), 4, 10, 6, 120, 5)
    n, m = len(node_image), len(src)
    d = [ctx.to_device(a, dt) for a, dt in ((node_image, np.int32), (src, np.int64), (dst, np.int64), (sim, np.float64))]
    out = dict(labels=ctx.empty((n,), np.int64), scores=ctx.empty((n,), np.float64), roots=ctx.empty((n,), np.uint8))
    n_tracks = C.c_int64(-1)
    _lib.check(ctx.lib.pxr_graph_labels_device(ctx.handle, n, d[0].ptr, m, d[1].ptr, d[2].ptr, d[3].ptr, out["labels"].ptr,
                                               out["scores"].ptr, out["roots"].ptr, C.byref(n_tracks)), "pxr_graph_labels_device")
    res = {k: v.download() for k, v in out.items()}
    res["n_tracks"] = n_tracks.value
    return res


def _extraction(ctx):
    """4096 patches of 8 x 8 x 64: the smallest count whose patches are walked in map-tile order, which the workspace holds."""
    import torch
    from pixsfm_amd.engine import PatchArena
    rng = np.random.default_rng(17)
    fmap = rng.normal(0, 1, (64, 48, 60)).astype(np.float32)
    kps = rng.uniform(-8, 250, (4096, 2))
    arena = PatchArena(ctx, len(kps), 8, 8, 64, np.float16)
    assert arena.extract(0, torch.from_numpy(fmap).cuda(), kps, (240.0, 192.0), l2_normalize=False) == len(kps)
    patches, corners, scales = arena.download()
    arena.close()
    return dict(patches=patches, corners=corners, scales=scales)


def _ka_solve(ctx):
    """A handful of sub-problems; 128 channels: its descriptor scratch alone is larger than all the layouts before it."""
    from pixsfm_amd import synthetic_ka
    from pixsfm_amd.engine import PatchArena, interp_cfg, make_loss
    from pixsfm_amd.ka_engine import KAProblem
    prob = synthetic_ka.make_ka_problem(n_tracks=6, track_len=4, seed=9, max_kps_per_problem=8)
    assert prob["n_problems"] >= 3
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ka = KAProblem(ctx, arena, prob)
    total, per = ka.solve(interp_cfg(), make_loss("cauchy", [0.25]), bound=4.0, per_problem=True)
    res = dict(keypoints=ka.keypoints())
    for key in sorted(per[0]):                                   # what the kernels report per sub-problem (no host timings)
        if not key.endswith("_ms"):
            res[key] = np.array([s[key] for s in per])
    arena.close()
    return res


def _positioning(ctx):
    """Global positioning on a ring of five images under the ground-truth rotations."""
    from pixsfm_amd.engine import GlobalPositioningProblem
    scene = gc.ring_scene(5, 3, 30, 7)
    b = gc.pair_directions(scene["qvec_gt"], scene["pair_image"], scene["pair_tvec"])
    gp = GlobalPositioningProblem(ctx, dict(scene, qvec=scene["qvec_gt"]), scene["pair_image"], b, scene["pair_weight"], 0)
    out = gp.solve()
    return {k: (v.download() if hasattr(v, "download") else v) for k, v in out.items()}


SEQUENCE = (_triangulation, _graph, _extraction, _ka_solve, _positioning, _triangulation)


def test_drivers_that_follow_each_other_on_one_context_compute_what_they_compute_alone():
    from pixsfm_amd.engine import Context
    alone = {}
    for stage in set(SEQUENCE):
        fresh = Context(0)
        alone[stage] = stage(fresh)
        fresh.close()
    shared = Context(0)
    try:
        for position, stage in enumerate(SEQUENCE):
            got, want = stage(shared), alone[stage]
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(got[key], want[key], equal_nan=True), (position, stage.__name__, key)
    finally:
        shared.close()
    # the runs are not vacuous: tracks were triangulated, patches extracted, keypoints moved, centres found
    assert (alone[_triangulation]["status"] == 0).any() and np.abs(alone[_extraction]["patches"]).max() > 0
    assert alone[_graph]["n_tracks"] > 0 and alone[_ka_solve]["num_successful"].sum() > 0
    assert alone[_positioning]["status"] == 0 and np.isfinite(alone[_positioning]["centre"]).all()
