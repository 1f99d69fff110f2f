"""The cases of the batched query bundle adjustment (pxr_query_ba_solve), shared by the lane-emulation test
and the GPU test: a batch whose queries sit on the edges of the kernel's mapping (16 residual blocks per workgroup pass at 128
channels), the oracle's solve of every query on its own, and the comparison.

A query is an image of synthetic.make_ba_problem with its perturbed pose and (some of) its observations; the points are the true
ones (`gt_xyz`), the references the points' (`refs`).  The oracle is pxo.ba_solve on the query's flat one-image problem, called as
tests/test_api_gpu.py::test_query_bundle_adjuster_like_pixsfm calls it."""
import functools

import numpy as np

# (image, number of its blocks taken from the front | None = all, correspondence that gets a second reference | None)
QUERIES = [(0, None, None), (1, None, None), (0, 1, None), (0, 3, None), (1, 15, None), (2, 16, None), (3, 17, None), (4, 33, None),
           (2, 0, None), (3, None, 3)]
# the duplicated correspondence's second reference (ref + 1e-3) leaves a cost floor of 0.5 C 1e-6 = 6.4e-5 at 128 channels: the
# full query that carries it is image 3's, whose initial cost (2.0) keeps that floor below 1e-4 of it (image 2's is 0.50)
FULL = (0, 1, 9)                 # the queries whose pose the correspondences determine well: held to the oracle's pose too
ORDER = [7, 2, 9, 4, 0, 8, 5, 3, 1, 6]      # the order of the batch: not the order of the sizes

# the project's own tolerances for a query BA against the oracle (test_query_bundle_adjuster_like_pixsfm)
INITIAL_COST_RTOL = 1e-10
FINAL_COST_TOL = 1e-6            # x the initial cost
POSE_ATOL = 1e-6


def _full(channels):
    from pixsfm_amd import synthetic
    more = {} if channels == 128 else {"channels": channels}
    return synthetic.make_ba_problem(n_cams=5, n_points=120, obs_per_point=3, seed=12, model=2, rot_deg=0.3, trans=0.02, **more)


def _query(full, image, count, dup):
    sel = np.nonzero(full["obs_image"] == image)[0]
    if count is not None:
        sel = sel[:count]
    patch, xyz, refs = [], [], []
    for i, o in enumerate(sel):
        pt = full["obs_point"][o]
        for d in ([full["refs"][pt], full["refs"][pt] + 1e-3] if dup == i else [full["refs"][pt]]):
            patch.append(o); xyz.append(full["gt_xyz"][pt]); refs.append(d)
    C = full["refs"].shape[1]
    return dict(image=image, obs_patch=np.asarray(patch, np.int64), xyz=np.asarray(xyz, np.float64).reshape(-1, 3),
                refs=np.asarray(refs, np.float64).reshape(-1, C), qvec=full["qvec"][image].copy(), tvec=full["tvec"][image].copy(),
                camera=int(full["image_camera"][image]))


@functools.lru_cache(maxsize=None)
def boundary_batch(channels=128):
    """-> (full problem, the queries in batch order, what QUERIES entry each is).  The arena of the batch is the full problem's
    (`patches`, `corners`, `scales`); a query's `obs_patch` indexes it."""
    full = _full(channels)
    queries = [_query(full, *QUERIES[k]) for k in ORDER]
    sizes = sorted(len(q["obs_patch"]) for q in queries)
    assert sizes[:7] == [0, 1, 3, 15, 16, 17, 33] and min(sizes[7:]) > 40, sizes
    return full, queries, list(ORDER)


def flatten(queries):
    """The arrays of pxr_query_ba_solve for a list of queries (one camera entry per query)."""
    C = next((q["refs"].shape[1] for q in queries), 0)
    off = np.concatenate([[0], np.cumsum([len(q["obs_patch"]) for q in queries])]).astype(np.int64)
    cat = lambda k, shape, dt: (np.concatenate([q[k] for q in queries]) if queries else np.zeros(0, dt)).astype(dt).reshape(shape)
    return dict(query_offsets=off, obs_patch=cat("obs_patch", (-1,), np.int64), xyz=cat("xyz", (-1, 3), np.float64),
                refs=cat("refs", (-1, C), np.float64), qvec=np.array([q["qvec"] for q in queries], np.float64).reshape(-1, 4),
                tvec=np.array([q["tvec"] for q in queries], np.float64).reshape(-1, 3),
                query_camera=np.array([q["camera"] for q in queries], np.int32))


@functools.lru_cache(maxsize=None)
def oracle(channels=128, loss=("cauchy", 0.25)):
    """The oracle's (summary, qvec, tvec) of every non-empty query of boundary_batch(channels), by position in the batch.  Every
    such solve converges well below its initial cost: a case that stops telling anything fails here."""
    import pxo
    full, queries, _ = boundary_batch(channels)
    out = []
    for q in queries:
        m = len(q["obs_patch"])
        if m == 0:
            out.append(None)
            continue
        cam = q["camera"]
        flat = dict(obs_image=np.zeros(m, np.int32), obs_point=np.arange(m, dtype=np.int32), obs_patch=np.arange(m, dtype=np.int64),
                    image_camera=np.zeros(1, np.int32), qvec=q["qvec"][None].copy(), tvec=q["tvec"][None].copy(),
                    cam_model=full["cam_model"][cam:cam + 1].copy(), cam_params=full["cam_params"][cam][None].copy(), xyz=q["xyz"],
                    refs=q["refs"], patches=np.ascontiguousarray(full["patches"][q["obs_patch"]]),
                    corners=full["corners"][q["obs_patch"]], scales=full["scales"][q["obs_patch"]])
        s, qo, to, _, _ = pxo.ba_solve(flat, pxo.cfg(), pxo.loss(*loss), [0], [0], [0b1111], np.ones(m, np.uint8), pxo.lm_options())
        assert s["termination"] == 0 and s["final_cost"] < 1e-4 * s["initial_cost"], (m, s)
        out.append((s, qo[0], to[0]))
    return out


def compare(got, channels=128, loss=("cauchy", 0.25), report=None):
    """got: per query of boundary_batch(channels), in batch order, (summary dict, qvec, tvec) of the code under test."""
    _, queries, kinds = boundary_batch(channels)
    ref = oracle(channels, loss)
    assert len(got) == len(queries)
    for i, (q, kind) in enumerate(zip(queries, kinds)):
        s, qv, tv = got[i]
        assert s["num_camera_unknowns"] == 6 and s["num_point_unknowns"] == 0 and s["accumulation"] == 2
        if ref[i] is None:                                          # the empty query keeps its pose
            assert s["iterations"] == 0 and s["termination"] == 0 and s["initial_cost"] == 0.0 and s["final_cost"] == 0.0
            assert np.array_equal(qv, q["qvec"]) and np.array_equal(tv, q["tvec"])
            continue
        so, qo, to = ref[i]
        d_init = abs(s["initial_cost"] - so["initial_cost"]) / so["initial_cost"]
        d_final = abs(s["final_cost"] - so["final_cost"]) / so["initial_cost"]
        d_pose = max(np.abs(qv - qo).max(), np.abs(tv - to).max())
        if report is not None:
            print("%squery %d (%d blocks): initial cost %.1e rel, final cost %.1e of initial, pose %.1e, iterations %d / %d, termination %d / %d"
                  % (report, kind, len(q["obs_patch"]), d_init, d_final, d_pose, s["iterations"], so["iterations"], s["termination"],
                     so["termination"]))
        assert d_init < INITIAL_COST_RTOL, (kind, d_init)
        assert d_final < FINAL_COST_TOL, (kind, d_final)
        assert s["termination"] == so["termination"], (kind, s, so)
        if kind in FULL:
            assert d_pose < POSE_ATOL, (kind, d_pose)


def same_bits(a, b):
    """Two results (summary dict, qvec, tvec) of one query: the same bits (total_ms is the launch's, not the query's)."""
    sa, sb = dict(a[0]), dict(b[0])
    sa.pop("total_ms"), sb.pop("total_ms")
    return sa == sb and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
