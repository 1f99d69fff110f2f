"""The SIFT kernels (csrc/pxr_sift.hip) on the GPU, through the C-ABI, against the numpy reference of tests/sift_cases.py.

Bounds.  The pyramid is held to the DERIVED bound of sift_cases.pass_bound: per pass (taps + 1) 2^-24 times the value range,
summed along the chain of passes that produced a level, computed from the radii.  eps = 8 x the largest bound of a case (a DoG is
a difference of two levels, times 4).  Every discrete decision of the reference carries a margin (sift_cases.detect /
orientations): a reference keypoint with margin > eps must appear with the same (o, s, xi, yi); every GPU keypoint must be a
reference candidate that is accepted or within eps of acceptance; at most 5 % of a case's reference keypoints (and orientations)
may have a margin <= eps -- asserted, the images and seeds of sift_gpu_cases.CASES were chosen on the CPU for it.

Refined values.  MEASURED on the reference alone (sift_cases.sensitivity: its pyramid moved by + or - the derived bound with random
signs, two seeds, over all cases of sift_gpu_cases.CASES), the largest change of each output: x / y 0.0635 px, sigma 4.93e-3
relative, response 8.05e-5, theta 0.0193 rad, a descriptor entry 1.67e-3.  Times 4:"""
import ctypes as C

import numpy as np
import pytest

import sift_cases as sc
import sift_gpu_cases as cases

pytestmark = pytest.mark.gpu

TOL_XY, TOL_SIGMA, TOL_RESPONSE, TOL_THETA, TOL_DESC = 4 * 0.0635, 4 * 4.93e-3, 4 * 8.05e-5, 4 * 0.0193, 4 * 1.67e-3


@pytest.fixture(scope="module")
def ctx():
    from pixsfm_amd.engine import Context
    return Context(0)


@pytest.fixture(scope="module")
def gpu(ctx):
    """name -> what the GPU gives for a case (computed once): pyramid, keypoints, record, response, descriptors, valid, found."""
    from pixsfm_amd.engine import SiftPyramid
    cache = {}

    def run(name):
        if name not in cache:
            r = cases.reference(name)
            pyr = SiftPyramid(ctx, r["image"], **r["kw"])
            kp, rec, resp, found = pyr.detect()
            desc, valid = pyr.describe(kp)
            cache[name] = dict(pyr=pyr, octaves=pyr.octaves(), kp=kp.download(), rec=rec.download(), resp=resp.download(),
                               desc=desc.download(), valid=valid.download(), found=found)
        return cache[name]
    return run


ALL = list(cases.CASES)


@pytest.mark.parametrize("name", ALL)
def test_pyramid_within_the_derived_bound(gpu, name):
    r, g = cases.reference(name), gpu(name)
    assert len(g["octaves"]) == len(r["pyr"])
    for k, (G, ref) in enumerate(zip(g["octaves"], r["pyr"])):
        assert G.shape == ref.shape
        for s in range(len(ref)):
            err = np.abs(G[s].astype(np.float64) - ref[s]).max()
            assert err <= r["bound"][k][s], (k, s, err, r["bound"][k][s])


@pytest.mark.parametrize("name", ALL)
def test_detection_against_the_reference_with_margins(gpu, name):
    r, g = cases.reference(name), gpu(name)
    eps = r["eps"]
    by_rec = {(c["o"], c["s"], c["xi"], c["yi"]): c for c in r["cands"]}
    accepted = [c for c in r["cands"] if c["accepted"]]
    if cases.CASES[name][2]:                                            # the condition on the reference alone
        assert sum(c["margin"] <= eps for c in accepted) <= 0.05 * len(accepted)
        assert (r["feats"]["orientation_margin"] <= eps).sum() <= 0.05 * len(r["feats"]["keypoints"])
    if name in cases.GRID_COUNTS:
        assert len(r["feats"]["keypoints"]) == cases.GRID_COUNTS[name] == g["found"]
    assert g["found"] == len(g["kp"])
    got = [tuple(int(v) for v in row) for row in g["rec"]]
    assert got == sorted(got, key=lambda t: (t[0], t[1], t[3], t[2]))     # ascending (o, s, yi, xi)
    got_set = set(got)
    for c in accepted:
        if c["margin"] > eps:
            assert (c["o"], c["s"], c["xi"], c["yi"]) in got_set, c
    for key in got_set:
        assert key in by_rec, key
        c = by_rec[key]
        assert c["accepted"] or c["reject_gap"] <= eps or c["path_margin"] <= eps, c
    # refined values and orientations of the keypoints both sides accept with every margin above eps
    rows = {}
    for i, key in enumerate(got):
        rows.setdefault(key, []).append(i)
    ref_rows = {}
    for i, rec in enumerate(r["feats"]["record"]):
        ref_rows.setdefault(tuple(int(v) for v in rec), []).append(i)
    compared = 0
    for key, ref_idx in ref_rows.items():
        c = by_rec[key]
        if key not in rows or c["margin"] <= eps:
            continue
        i0, j0 = ref_idx[0], rows[key][0]
        a, b = r["feats"]["keypoints"][i0], g["kp"][j0]
        assert abs(a[0] - b[0]) <= TOL_XY and abs(a[1] - b[1]) <= TOL_XY, (key, a, b)
        assert abs(b[2] / a[2] - 1.0) <= TOL_SIGMA
        assert abs(r["feats"]["response"][i0] - g["resp"][j0]) <= TOL_RESPONSE
        compared += 1
        if r["feats"]["orientation_margin"][i0] <= eps:
            continue
        assert len(rows[key]) == len(ref_idx), key
        for i, j in zip(ref_idx, rows[key]):
            dth = abs(r["feats"]["keypoints"][i][3] - g["kp"][j][3])
            assert min(dth, 2 * np.pi - dth) <= TOL_THETA, key
    assert compared > 0


@pytest.mark.parametrize("name", ALL)
def test_descriptors_of_the_gpus_own_keypoints(gpu, name):
    """The reference is given the GPU's own (x, y, sigma, theta), so only the pyramid's rounding separates the two."""
    r, g = cases.reference(name), gpu(name)
    ref, valid = sc.describe(r["pyr"], r["opt"], g["kp"])
    assert np.array_equal(g["valid"].astype(bool), valid) and valid.all()
    assert np.abs(g["desc"] - ref).max() <= TOL_DESC
    assert np.abs(np.linalg.norm(g["desc"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize("name", ["65x63_u8", "grid_257", "view_320"])
def test_two_runs_give_identical_bits(ctx, gpu, name):
    from pixsfm_amd.engine import SiftPyramid
    r, g = cases.reference(name), gpu(name)
    pyr = SiftPyramid(ctx, r["image"], **r["kw"])
    kp, rec, resp, found = pyr.detect()
    desc, valid = pyr.describe(kp)
    assert found == g["found"]
    assert all(np.array_equal(a, b) for a, b in zip(pyr.octaves(), g["octaves"]))
    for a, b in ((kp, "kp"), (rec, "rec"), (resp, "resp"), (desc, "desc"), (valid, "valid")):
        assert a.download().tobytes() == g[b].tobytes(), b


@pytest.mark.parametrize("name", ["grid_65", "view_320"])
def test_capacity_below_the_number_found(ctx, gpu, name):
    g = gpu(name)
    n = g["found"]
    for cap in (0, 1, n // 2, n - 1):
        kp, rec, resp = ctx.to_device(np.full((n + 4, 4), -9.0)), ctx.to_device(np.full((n + 4, 4), -9, np.int32)), ctx.to_device(np.full(n + 4, -9.0, np.float32))
        _, _, _, found = g["pyr"].detect(capacity=cap, out=(kp, rec, resp))
        assert found == n
        kp, rec, resp = kp.download(), rec.download(), resp.download()
        assert np.array_equal(kp[:cap], g["kp"][:cap]) and np.array_equal(rec[:cap], g["rec"][:cap]) and np.array_equal(resp[:cap], g["resp"][:cap])
        assert (kp[cap:] == -9).all() and (rec[cap:] == -9).all() and (resp[cap:] == -9).all()


def test_both_dtypes_and_a_constant_image(ctx):
    from pixsfm_amd.engine import SiftPyramid
    u8 = sc.oriented_scene(65, 63, 1, dtype=np.uint8)
    f32 = u8.astype(np.float32) / np.float32(255)
    a, b = SiftPyramid(ctx, u8), SiftPyramid(ctx, f32)
    assert a.d_pyramid.download().tobytes() == b.d_pyramid.download().tobytes()
    flat = SiftPyramid(ctx, np.full((40, 50), 100, np.uint8))
    assert flat.detect()[3] == 0
    assert SiftPyramid(ctx, np.full((7, 9), 3, np.uint8)).detect()[3] == 0          # no octave at all


def _opts(**kw):
    from pixsfm_amd.engine import sift_options
    return sift_options(**kw)


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(ctx, gpu):
    g = gpu("64x64_octave0")
    pyr = g["pyr"]
    lib, h, w = ctx.lib, 64, 64
    image = ctx.to_device(cases.reference("64x64_octave0")["image"])
    n_flat = pyr.d_pyramid.shape[0]
    bad = [dict(first_octave=1), dict(first_octave=-2), dict(octave_resolution=1), dict(octave_resolution=5),
           dict(sigma0=1.0, first_octave=-1), dict(sigma0=0.5, first_octave=0), dict(num_octaves=-1), dict(num_octaves=9),
           dict(num_octaves=4, first_octave=0), dict(max_num_orientations=0), dict(max_num_orientations=5)]
    sent = np.full(n_flat, -7.0, np.float32)
    for kw in bad:
        o = _opts(**kw)
        nbytes, found = C.c_int64(-9), C.c_int64(-9)
        assert lib.pxr_sift_pyramid_bytes(h, w, C.byref(o), C.byref(nbytes)) == -1 and nbytes.value == -9, kw
        d = ctx.to_device(sent)
        assert lib.pxr_sift_pyramid(ctx.handle, image.ptr, 1, h, w, C.byref(o), d.ptr) == -1, kw
        assert (d.download() == -7).all(), kw
        kp, rec, resp = ctx.to_device(np.full((8, 4), -9.0)), ctx.to_device(np.full((8, 4), -9, np.int32)), ctx.to_device(np.full(8, -9.0, np.float32))
        assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), 8, kp.ptr, rec.ptr, resp.ptr, C.byref(found)) == -1, kw
        assert found.value == -9 and (kp.download() == -9).all() and (rec.download() == -9).all() and (resp.download() == -9).all()
        desc, valid = ctx.to_device(np.full((2, 128), -9.0, np.float32)), ctx.to_device(np.full(2, 9, np.uint8))
        assert lib.pxr_sift_describe(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), 2, kp.ptr, desc.ptr, valid.ptr) == -1, kw
        assert (desc.download() == -9).all() and (valid.download() == 9).all()
    o = _opts(first_octave=0)
    found = C.c_int64(-9)
    kp, rec, resp = ctx.to_device(np.full((8, 4), -9.0)), ctx.to_device(np.full((8, 4), -9, np.int32)), ctx.to_device(np.full(8, -9.0, np.float32))
    for hh, ww in ((0, 64), (64, 0), (-3, 64)):
        assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, hh, ww, C.byref(o), 8, kp.ptr, rec.ptr, resp.ptr, C.byref(found)) == -1
    assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), -1, kp.ptr, rec.ptr, resp.ptr, C.byref(found)) == -1
    assert lib.pxr_sift_detect(ctx.handle, None, h, w, C.byref(o), 8, kp.ptr, rec.ptr, resp.ptr, C.byref(found)) == -1
    assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), 8, None, rec.ptr, resp.ptr, C.byref(found)) == -1
    assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), 8, kp.ptr, rec.ptr, resp.ptr, None) == -1
    assert lib.pxr_sift_detect(ctx.handle, pyr.d_pyramid.ptr, h, w, None, 8, kp.ptr, rec.ptr, resp.ptr, C.byref(found)) == -1
    assert lib.pxr_sift_describe(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), -1, kp.ptr, None, None) == -1
    assert lib.pxr_sift_describe(ctx.handle, pyr.d_pyramid.ptr, h, w, C.byref(o), 2, None, None, None) == -1
    assert lib.pxr_sift_pyramid(ctx.handle, None, 1, h, w, C.byref(o), pyr.d_pyramid.ptr) == -1
    assert lib.pxr_sift_pyramid(ctx.handle, image.ptr, 2, h, w, C.byref(o), pyr.d_pyramid.ptr) == -1
    assert found.value == -9 and (kp.download() == -9).all() and (rec.download() == -9).all() and (resp.download() == -9).all()


def test_keypoints_that_cannot_be_described(gpu):
    """NaN, infinite, non-positive or out-of-range sigma, positions far outside: valid = 0 and zeros, never a fault, and the
    neighbours in the same launch are unaffected."""
    g = gpu("97x131_three_octaves")
    good = g["kp"][:6]
    nan, inf = np.nan, np.inf
    bad = np.array([[nan, 3, 2, 0], [3, inf, 2, 0], [3, 3, -1, 0], [3, 3, 0, 0], [3, 3, 2, nan], [3, 3, 1e-3, 0], [3, 3, 1e6, 0],
                    [1e300, -1e300, 2, 0], [-500, 20, 2, 0], [3, 3, inf, 0]])
    mixed, kinds = [], []
    for i in range(max(len(good), len(bad))):
        if i < len(good):
            mixed.append(good[i]); kinds.append(("g", i))
        if i < len(bad):
            mixed.append(bad[i]); kinds.append(("b", i))
    desc, valid = g["pyr"].describe(np.array(mixed))
    desc, valid = desc.download(), valid.download()
    for row, (kind, i) in enumerate(kinds):
        if kind == "g":
            assert valid[row] == 1 and np.array_equal(desc[row], g["desc"][i])
        else:
            assert valid[row] == 0 and (desc[row] == 0).all(), bad[i]


def test_descriptors_go_to_the_matcher_as_device_pointers(ctx, gpu):
    """pxr_match_descriptors on the descriptor buffers of two images where pxr_sift_describe left them gives the same bits as on
    the same descriptors uploaded from the host."""
    from pixsfm_amd.engine import MatchProblem
    a, b = gpu("grid_65"), gpu("view_320")
    da, db = a["pyr"].describe(a["kp"])[0], b["pyr"].describe(b["kp"])[0]
    both = ctx.empty((da.shape[0] + db.shape[0], 128), np.float32)
    # the flat descriptor array of a batch is one allocation, so the two images are described straight into its two halves
    out_a = (_view(ctx, both, 0, da.shape[0]), ctx.empty((da.shape[0],), np.uint8))
    out_b = (_view(ctx, both, da.shape[0], db.shape[0]), ctx.empty((db.shape[0],), np.uint8))
    a["pyr"].describe(a["kp"], out=out_a)
    b["pyr"].describe(b["kp"], out=out_b)
    offsets = np.array([0, da.shape[0], da.shape[0] + db.shape[0]], np.int64)
    pairs = [(0, 1), (1, 0), (0, 0)]
    on_device = MatchProblem(ctx, both, pairs, image_offsets=offsets).run(ratio_threshold=0.8)
    from_host = MatchProblem(ctx, np.concatenate([a["desc"], b["desc"]]), pairs, image_offsets=offsets).run(ratio_threshold=0.8)
    for x, y in zip(on_device, from_host):
        assert x.download().tobytes() == y.download().tobytes()
    assert on_device[2].download()[2] == da.shape[0]                      # an image against itself: every feature finds itself


def _view(ctx, array, first, rows):
    """Rows [first, first + rows) of a device array as a device array that does not own the memory."""
    from pixsfm_amd.engine import DeviceArray
    v = DeviceArray.__new__(DeviceArray)
    v.ctx, v.shape, v.dtype = ctx, (rows,) + tuple(array.shape[1:]), array.dtype
    v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize
    v.ptr = C.c_void_p(array.ptr.value + first * int(np.prod(array.shape[1:], dtype=np.int64)) * array.dtype.itemsize)
    v.free = lambda: None
    v._keep = array
    return v
