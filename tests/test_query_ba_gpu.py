"""GPU: the batched query bundle adjustment (pxr_query_ba_solve) against the oracle's solve of every query
on the boundary batch of tests/query_ba_cases.py, its bit-for-bit properties, its argument checks, and the Python layers on top
of it: QueryBundleOptimizer.run_batch against run(), QueryLocalizer.localize_batch against localize() on the scene of
tests/test_query_localizer_gpu.py with three held-out images, MapLocalizer's "refine_batch" on the map of two rings."""
import ctypes as C
from copy import deepcopy

import numpy as np
import pytest

import query_ba_cases as qc

pytestmark = pytest.mark.gpu

_ARENAS = {}


def _arena(ctx, channels):
    from pixsfm_amd.engine import PatchArena
    if channels not in _ARENAS:
        full = qc.boundary_batch(channels)[0]
        _ARENAS[channels] = PatchArena.from_numpy(ctx, full["patches"], full["corners"], full["scales"])
    return _ARENAS[channels]


def _solve(ctx, channels, queries, loss=("cauchy", 0.25), **change):
    """pxr_query_ba_solve on `queries` over the arena of boundary_batch(channels) -> per query (summary dict, qvec, tvec)."""
    from pixsfm_amd.engine import QueryBAProblem, interp_cfg, lm_options, make_loss
    full = qc.boundary_batch(channels)[0]
    prob = dict(qc.flatten(queries), cam_model=full["cam_model"], cam_params=full["cam_params"])
    prob.update(change)
    qba = QueryBAProblem(ctx, _arena(ctx, channels), prob)
    per = qba.solve(interp_cfg(), make_loss(loss[0], [loss[1]]), lm_options(), timed=True)
    assert set(qba.kernel_ms) == {"solve"} and all(s["total_ms"] == per[0]["total_ms"] for s in per)
    q, t = qba.poses()
    return [(per[i], q[i], t[i]) for i in range(len(queries))]


@pytest.fixture(scope="module")
def batch_results(ctx):
    return {ch: _solve(ctx, ch, qc.boundary_batch(ch)[1]) for ch in (128, 64)}


@pytest.mark.parametrize("channels", [128, 64])
def test_the_boundary_batch_matches_the_oracle(batch_results, channels, capsys):
    with capsys.disabled():
        qc.compare(batch_results[channels], channels, report="GPU vs oracle, C = %d: " % channels)


@pytest.mark.parametrize("channels", [128, 64])
def test_same_bits_on_every_run_alone_and_in_the_reversed_batch(ctx, batch_results, channels):
    queries = qc.boundary_batch(channels)[1]
    got = batch_results[channels]
    again = _solve(ctx, channels, queries)
    rev = _solve(ctx, channels, queries[::-1])[::-1]
    for i, q in enumerate(queries):
        assert qc.same_bits(again[i], got[i]), "position %d, second run" % i
        assert qc.same_bits(rev[i], got[i]), "position %d in the reversed batch" % i
        assert qc.same_bits(_solve(ctx, channels, [q])[0], got[i]), "position %d alone" % i


def test_invalid_arguments_leave_every_output_untouched(ctx):
    from pixsfm_amd._lib import LMSummary, PixsfmHipError
    from pixsfm_amd.engine import QueryBAProblem, interp_cfg, lm_options, make_loss
    full, queries, _ = qc.boundary_batch(128)
    queries = [queries[1], queries[5], queries[3]]                  # 1, 0 and 15 blocks
    f = qc.flatten(queries)
    off = f["query_offsets"]
    bad_patch, neg_patch = f["obs_patch"].copy(), f["obs_patch"].copy()
    bad_patch[-1], neg_patch[0] = len(full["patches"]), -1
    for change, word in ((dict(query_offsets=np.array([0, 5, off[2], off[3]], np.int64)), "monotone"),
                         (dict(query_offsets=np.array([1, off[1], off[2], off[3]], np.int64)), "not 0"),
                         (dict(query_offsets=np.array([0, off[1], off[2], off[3] - 1], np.int64)), "n_obs"),
                         (dict(query_camera=np.array([0, len(full["cam_model"]), 0], np.int32)), "camera"),
                         (dict(obs_patch=bad_patch), "patch"), (dict(obs_patch=neg_patch), "patch")):
        prob = dict(f, cam_model=full["cam_model"], cam_params=full["cam_params"])
        prob.update(change)
        qba = QueryBAProblem(ctx, _arena(ctx, 128), prob)
        summaries = (LMSummary * 3)()
        C.memset(summaries, 0x5a, C.sizeof(summaries))
        before = bytes(summaries)
        cfg, ls, opt, d = interp_cfg(), make_loss("cauchy", [0.25]), lm_options(), qba.d
        rc = ctx.lib.pxr_query_ba_solve(ctx.handle, qba.arena.handle, 3, d["query_offsets"].ptr, qba.n_obs, d["obs_patch"].ptr, d["xyz"].ptr,
                                        d["refs"].ptr, d["query_camera"].ptr, qba.n_cameras, d["cam_model"].ptr, d["cam_params"].ptr,
                                        d["qvec"].ptr, d["tvec"].ptr, C.byref(cfg), C.byref(ls), C.byref(opt), summaries)
        assert rc == -1 and word in ctx.lib.pxr_last_error().decode(), (word, rc, ctx.lib.pxr_last_error())
        q, t = qba.poses()
        assert np.array_equal(q, f["qvec"]) and np.array_equal(t, f["tvec"]) and bytes(summaries) == before
        with pytest.raises(PixsfmHipError, match=word):
            qba.solve(cfg, ls, opt)
    prob = dict(f, cam_model=full["cam_model"], cam_params=full["cam_params"])
    qba = QueryBAProblem(ctx, _arena(ctx, 128), prob)
    d = qba.d
    rc = ctx.lib.pxr_query_ba_solve(ctx.handle, None, 3, d["query_offsets"].ptr, qba.n_obs, d["obs_patch"].ptr, d["xyz"].ptr, d["refs"].ptr,
                                    d["query_camera"].ptr, qba.n_cameras, d["cam_model"].ptr, d["cam_params"].ptr, d["qvec"].ptr, d["tvec"].ptr,
                                    C.byref(interp_cfg()), C.byref(make_loss()), C.byref(lm_options()), (LMSummary * 3)())
    assert rc == -1 and "NULL" in ctx.lib.pxr_last_error().decode()


# ---- QueryBundleOptimizer.run_batch ------------------------------------------------------------------------------------------------
def _api_queries(channels=128):
    """The three full queries of the boundary batch as run() takes them: (qvec, tvec, camera, points3D, fmap, references) + oracle."""
    from pixsfm_amd.api import features
    from pixsfm_amd.api.reconstruction import Camera
    full, queries, kinds = qc.boundary_batch(channels)
    ref = qc.oracle(channels)
    out = []
    for i, (q, kind) in enumerate(zip(queries, kinds)):
        if kind not in qc.FULL:
            continue
        image, _, dup = qc.QUERIES[kind]
        sel = np.nonzero(full["obs_image"] == image)[0]
        pts = full["obs_point"][sel]
        refs = [full["refs"][p].copy() for p in pts]
        if dup is not None:
            refs[dup] = [refs[dup], refs[dup] + 1e-3]
        fmap = features.FeatureMap.from_arrays(full["patches"][sel], np.arange(len(sel)), full["corners"][sel], (1.0, 1.0))
        cam = Camera(1, 2, 1000, 1000, full["cam_params"][q["camera"], :4].copy())
        out.append(dict(args=lambda q=q, cam=cam, pts=pts, fmap=fmap, refs=refs: (q["qvec"].copy(), q["tvec"].copy(), deepcopy(cam),
                                                                                    [full["gt_xyz"][p].copy() for p in pts], fmap, refs),
                        oracle=ref[i]))
    assert len(out) == 3
    return out


def test_run_batch_against_run_on_the_full_queries(ctx):
    from pixsfm_amd.api import QueryBundleAdjuster
    cases = _api_queries()
    single, per_query = [], QueryBundleAdjuster(ctx=ctx)
    for c in cases:
        a = c["args"]()
        assert per_query.refine(*a)
        single.append((a, per_query.solver.last_summary))
    adj = QueryBundleAdjuster(ctx=ctx)
    batch = [c["args"]() for c in cases]
    starts = [(b[0].copy(), b[1].copy()) for b in batch]
    assert adj.refine_batch(batch) == [True] * 3 and adj.solver.last_batch_path == "batch"
    for k, (c, b, start, (a, s)) in enumerate(zip(cases, batch, starts, single)):
        so, qo, to = c["oracle"]
        sb = adj.solver.last_summaries[k]
        assert not np.array_equal(b[0], start[0]) and not np.array_equal(b[1], start[1])          # refined in place
        assert np.abs(b[0] - qo).max() < 1e-6 and np.abs(b[1] - to).max() < 1e-6                   # both are within 1e-6 of the oracle,
        assert np.abs(b[0] - a[0]).max() < 2e-6 and np.abs(b[1] - a[1]).max() < 2e-6               # hence within 2e-6 of each other
        assert abs(sb["final_cost"] - s["final_cost"]) < 2e-6 * so["initial_cost"]
        assert sb["num_camera_unknowns"] == 6 and sb["termination"] == so["termination"]
    # a query without residuals next to one with: False, its pose untouched
    a, b = cases[0]["args"](), cases[1]["args"]()
    q0, t0 = a[0].copy(), a[1].copy()
    assert adj.refine_batch([a + ([False] * len(a[3]),), b]) == [False, True]
    assert np.array_equal(a[0], q0) and np.array_equal(a[1], t0) and adj.solver.last_summaries[0] is None
    assert np.array_equal(b[0], batch[1][0])                                                       # and the other one's bits are the batch's


def test_run_batch_falls_back_to_run_with_the_same_bits(ctx):
    from pixsfm_amd.api import QueryBundleAdjuster
    cases = _api_queries()[:2]
    conf = {"optimizer": {"refine_focal_length": True}}
    single = []
    for c in cases:
        a = c["args"]()
        assert QueryBundleAdjuster(conf, ctx=ctx).refine(*a)
        single.append(a)
    adj = QueryBundleAdjuster(conf, ctx=ctx)
    batch = [c["args"]() for c in cases]
    assert adj.refine_batch(batch) == [True, True] and adj.solver.last_batch_path == "per_query"
    for a, b in zip(single, batch):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].params, b[2].params)
        assert b[2].params[0] != 1200.0                                                            # the focal length moved
    assert adj.solver.last_summaries[1]["num_camera_unknowns"] == 7


# ---- QueryLocalizer.localize_batch: the scene of tests/test_query_localizer_gpu.py with three held-out images ---------------------
N_CAMS, N_POINTS, N_HELD = 11, 100, 3


def make_scene(ctx):
    from pixsfm_amd import synthetic
    from pixsfm_amd.api import QueryLocalizer, features
    from pixsfm_amd.api.reconstruction import Camera, reconstruction_from_flat
    full = synthetic.make_ba_problem(n_cams=N_CAMS, n_points=N_POINTS, obs_per_point=5, channels=64, patch_size=16, seed=61,
                                     perturb=False, shared_camera=True)
    held = full["obs_image"] < N_HELD                            # images 0 .. 2 are the queries; the map is what the others see
    m = ~held
    flat = dict(full, obs_image=full["obs_image"][m] - N_HELD, obs_point=full["obs_point"][m], obs_patch=full["obs_patch"][m],
                centers=full["centers"][m], image_camera=full["image_camera"][N_HELD:], qvec=full["qvec"][N_HELD:], tvec=full["tvec"][N_HELD:])
    rec, patch_of = reconstruction_from_flat(flat)
    fmaps = {}
    for (image_id, p2d), pi in patch_of.items():
        fm = fmaps.setdefault(rec.images[image_id].name, features.FeatureMap())
        fm.patches[p2d] = features.FeaturePatch(full["patches"][pi], full["corners"][pi], full["scales"][pi])
    manager = features.FeatureManager([features.FeatureSet(fmaps)])
    in_map = set(int(p) for p in full["obs_point"][m])
    # per query: keypoints up to 1.5 px off their true place, one right pair each, and a quarter as many wrong pairs on top
    # (20 % of all), each re-using a keypoint and a 3D point that also have their right pair
    rng = np.random.default_rng(62)
    queries = []
    for image in range(N_HELD):
        sel = np.array([o for o in np.flatnonzero(full["obs_image"] == image) if int(full["obs_point"][o]) in in_map])
        nq = len(sel)
        assert nq >= 30
        keypoints = full["centers"][sel] + rng.uniform(-1.5, 1.5, (nq, 2))
        kp_idx, p3d_id, wrong = list(range(nq)), [int(p) + 1 for p in full["obs_point"][sel]], [False] * nq
        for i in rng.permutation(nq)[:nq // 4]:
            far = [j for j in range(nq) if np.linalg.norm(full["centers"][sel[j]] - full["centers"][sel[i]]) > 60.0]
            kp_idx.append(int(i)); p3d_id.append(p3d_id[int(rng.choice(far))]); wrong.append(True)
        fmap = features.FeatureMap.from_arrays(full["patches"][sel], np.arange(nq), full["corners"][sel], (1.0, 1.0))
        queries.append(dict(keypoints=keypoints, kp_idx=kp_idx, p3d_id=p3d_id, wrong=np.array(wrong), fmap=fmap,
                            gt_q=full["gt_qvec"][image], gt_t=full["gt_tvec"][image]))
    camera = Camera(1, 2, 1000, 1000, full["cam_params"][0, :4].copy())
    localizer = QueryLocalizer(rec, None, dense_features=manager, ctx=ctx)           # option 2: references from the map's features
    return dict(rec=rec, localizer=localizer, queries=queries, camera=camera)


@pytest.fixture(scope="module")
def scene(ctx):
    return make_scene(ctx)


def _pose_error(s, pose):
    from pixsfm_amd import synthetic
    R0, R1 = synthetic.qvec_to_rotmat(s["gt_q"]), synthetic.qvec_to_rotmat(pose["qvec"])
    ang = np.arccos(np.clip((np.trace(R0.T @ R1) - 1.0) / 2.0, -1.0, 1.0))
    return float(ang), float(np.linalg.norm(-R0.T @ s["gt_t"] + R1.T @ pose["tvec"]))


def _as_dict(scene, s):
    return dict(keypoints=s["keypoints"].copy(), pnp_point2D_idxs=s["kp_idx"], pnp_points3D_id=s["p3d_id"],
                query_camera=deepcopy(scene["camera"]), query_fmaps=[s["fmap"]])


def test_localize_batch_against_localize(scene):
    loc = scene["localizer"]
    qs = scene["queries"]
    single = [loc.localize(s["keypoints"].copy(), s["kp_idx"], s["p3d_id"], deepcopy(scene["camera"]), query_fmaps=[s["fmap"]]) for s in qs]
    # dicts and tuples, a query without pairs in the middle and one whose pairs are all wrong at the end
    lost = dict(qs[0], p3d_id=[qs[0]["p3d_id"][(k * 7 + 11) % len(qs[0]["wrong"])] if not w else p
                               for k, (p, w) in enumerate(zip(qs[0]["p3d_id"], qs[0]["wrong"]))])
    lost_single = loc.localize(lost["keypoints"].copy(), lost["kp_idx"], lost["p3d_id"], deepcopy(scene["camera"]), query_fmaps=[lost["fmap"]])
    batch = [_as_dict(scene, qs[0]), (qs[1]["keypoints"].copy(), qs[1]["kp_idx"], qs[1]["p3d_id"], deepcopy(scene["camera"]), None, [qs[1]["fmap"]]),
             dict(_as_dict(scene, qs[2]), pnp_point2D_idxs=[], pnp_points3D_id=[]), _as_dict(scene, qs[2]), _as_dict(scene, lost)]
    out = loc.localize_batch(batch)
    assert loc.query_bundle_adjuster.solver.last_batch_path == "batch"
    assert len(out) == 5 and out[2] == {"success": False}
    assert out[4]["success"] == lost_single["success"] and (lost_single["success"] or out[4] == lost_single)
    for s, one, got in zip(qs, single, [out[0], out[1], out[3]]):
        assert one["success"] and got["success"] and set(got) == set(one)
        assert got["inliers"] == one["inliers"] and got["num_inliers"] == one["num_inliers"]
        assert not np.array(got["inliers"])[s["wrong"]].any()
        e1, e0 = _pose_error(s, got), _pose_error(s, one)
        print("pose error (rad, centre): localize_batch %.3e %.3e, localize %.3e %.3e" % (e1 + e0))
        assert e1[0] <= 2 * e0[0] and e1[1] <= 2 * e0[1]                                           # twice this query's per-query figure
    alone = loc.localize_batch([_as_dict(scene, qs[1])])[0]
    assert alone["qvec"].tobytes() == out[1]["qvec"].tobytes() and alone["tvec"].tobytes() == out[1]["tvec"].tobytes()
    assert alone["inliers"] == out[1]["inliers"]


# ---- MapLocalizer: "refine_batch" on the map of two rings (tests/test_map_localization_gpu.py) ------------------------------------
MATCHER = {"distance_threshold": 0.7}      # true matches have distance 0, random unit descriptors about 1.4


def _map_pose_error(qvec, tvec, truth):
    from pixsfm_amd import synthetic
    R, Rt = synthetic.qvec_to_rotmat(qvec), synthetic.qvec_to_rotmat(truth[0])
    rot = np.degrees(np.arccos(np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)))
    return float(rot), float(np.linalg.norm(-R.T @ tvec + Rt.T @ truth[1]))


def test_map_localizer_refines_in_one_batch(ctx):
    """The map of two rings has keypoints and descriptors but no feature patches: the QueryLocalizer that refines runs its PnP, the
    unique inliers and the recount (QKA and QBA are off) -- through localize() per query by default, through one localize_batch
    call with "refine_batch"."""
    import map_localization_cases as lc
    from pixsfm_amd.api import MapLocalizer, QueryLocalizer
    tp = lc.two_places()
    rec, scene, queries = tp["reconstruction"], tp["scene"], tp["queries"]
    cameras = {q: scene["camera"] for q in queries}
    refine = QueryLocalizer(rec, {"QKA": {"apply": False}, "QBA": {"apply": False}}, ctx=ctx)
    calls = []
    localize, localize_batch = refine.localize, refine.localize_batch
    refine.localize = lambda *a, **k: calls.append("localize") or localize(*a, **k)
    refine.localize_batch = lambda qs: calls.append("localize_batch %d" % len(qs)) or localize_batch(qs)
    plain = MapLocalizer(rec, {"matcher": MATCHER}, ctx=ctx).localize_queries(cameras, scene["keypoints"], tp["descriptors"], tp["retrieval"])
    loop = MapLocalizer(rec, {"matcher": MATCHER, "refine": refine}, ctx=ctx).localize_queries(cameras, scene["keypoints"], tp["descriptors"],
                                                                                             tp["retrieval"])
    assert calls == ["localize"] * 4
    del calls[:]
    one = MapLocalizer(rec, {"matcher": MATCHER, "refine": refine, "refine_batch": True}, ctx=ctx).localize_queries(
        cameras, scene["keypoints"], tp["descriptors"], tp["retrieval"])
    assert calls[0] == "localize_batch 4" and "localize" not in calls
    for q in queries:
        assert plain[q]["success"] and loop[q]["success"] and one[q]["success"]
        assert one[q]["num_inliers"] == loop[q]["num_inliers"] and one[q]["inliers"] == loop[q]["inliers"]
        ref_rot, ref_centre = _map_pose_error(loop[q]["qvec"], loop[q]["tvec"], scene["poses"][q])
        rot, centre = _map_pose_error(one[q]["qvec"], one[q]["tvec"], scene["poses"][q])
        assert rot <= 2 * ref_rot and centre <= 2 * ref_centre
        assert np.array_equal(one[q]["point2D_idxs"], plain[q]["point2D_idxs"])
