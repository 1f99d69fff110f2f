"""GPU: every combination an entry point's dispatch enumerates (csrc/pxr_dispatch.h: storage x channels x output storage x
flag) launches the kernel of THAT combination.

Each call runs through the C ABI at the smallest shape its kernel takes and is compared with the same call on the same values
stored as fp64 (the fp64 kernel of the same channel count); where no fp64 kernel exists, with the numpy statement the entry
point's own test uses.  Tolerances are those tests' (named at each check) and conftest's FP32_PASS_*: the descriptor kernels
of fp16 / fp32 storage run the reference's fp32 horizontal pass and the fp64 ones do not, so across that pass (1.4e-8 .. 2.2e-8 on
unit descriptors, measured) a combination is held to conftest's price of it, and the fp16 arena also to the fp32 arena at the tight
tolerances.  The inputs lie on a grid of 2^-8 (exact in fp16, and so are their differences: the cost-map kernels subtract in
the storage type), so the storage types differ by their arithmetic only; a launch of the wrong storage type, channel count or
output type reads or writes with the wrong stride and misses these tolerances by orders of magnitude.  Per site, one arena it
does not support must be refused with the status code it has always returned.

Left out (rejected by design, not by this file):
  * k_gram_build / k_inner_gram_packed / k_inner_packed with fp64 storage: fp64 arenas take pxr_ba_eval and k_inner_points
    (gram_eval_supported, launch_inner_iterations); those are the fp64 references here.
  * costmap_interp_kernel with 3 / 1 channels: pxr_costmap_extract_ex answers PXR_EUNSUPPORTED (checked below).
  * extract_kernel / dsift kernels with an fp64 source: pxr_arena_extract / ds_check answer PXR_EUNSUPPORTED (checked below).
  * pxr_ka_* with 3 channels: ka_kernels has 128, 64 and 1 (PXR_EUNSUPPORTED is checked for 32).

`python tests/test_dispatch_matrix_gpu.py` prints one SHA-256 of the output bytes per combination (the same matrix): two builds
that dispatch alike print the same listing."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsift_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
STORAGES = (F16, F32, F64)
NAME = {F16: "f16", F32: "f32", F64: "f64", np.uint8: "u8"}
# tests/test_dsift_gpu.py
DENSE_ATOL, ROOTSIFT_ATOL = 1e-6, 5e-4
PS = 8


def _grid(a):
    """Onto multiples of 2^-8: below 1 in magnitude these, and their differences, are exact in fp16."""
    return np.round(np.asarray(a, np.float64) * 256.0) / 256.0


# ---- inputs (host, made once) ----------------------------------------------------------------------------------------------------
TRACKS = (18, 12, 8)   # point p is seen by images 0 .. TRACKS[p] - 1


@functools.lru_cache(maxsize=None)
def _scene(channels, ps=PS):
    """18 images on 2 cameras, 3 points with tracks of 18 (beyond IG_MAXO = 16: the long-track kernel), 12 and 8 observations
    (REF_REG_TRACK = 8: k_irls keeps that one in registers); one patch per observation.  The solves need poses that are held by
    three points and points that are held by constant poses, hence 38 observations rather than a handful.
    One channel: the first of three (a normalised single channel would be +-1)."""
    from pixsfm_amd import synthetic
    p = synthetic.make_ba_problem(n_cams=18, n_points=3, obs_per_point=18, channels=max(channels, 3), patch_size=ps, seed=3,
                                  dtype=F64, rot_deg=0.02, trans=0.001, pt_sigma=0.003)
    keep = p["obs_image"] < np.asarray(TRACKS)[p["obs_point"]]
    for k in ("obs_image", "obs_point", "patches", "corners", "scales", "centers"):
        p[k] = p[k][keep]
    p["obs_patch"] = np.arange(keep.sum(), dtype=np.int64)
    p["image_camera"] = (np.arange(18) % 2).astype(np.int32)
    p["cam_model"], p["cam_params"] = p["cam_model"][:2], p["cam_params"][:2]
    p["patches"], p["refs"] = _grid(p["patches"][..., :channels]), _grid(p["refs"][:, :channels])
    return p


def _cfg(channels, **kw):
    """Descriptors are normalised, intensities and cost maps are not (a normalised single channel is +-1)."""
    from pixsfm_amd.engine import interp_cfg
    return interp_cfg(l2_normalize=channels >= 64, **kw)


def _arena(ctx, scene, st):
    from pixsfm_amd.engine import PatchArena
    return PatchArena.from_numpy(ctx, scene["patches"].astype(st), scene["corners"], scene["scales"])


def _ba(ctx, st, channels, ps=PS):
    from pixsfm_amd.engine import BAProblem
    scene = _scene(channels, ps)
    return scene, BAProblem(ctx, _arena(ctx, scene, st), scene)


def _loss():
    from pixsfm_amd.engine import make_loss
    return make_loss("cauchy", [0.25])


def _gauge(scene):
    """Images 1 and 2 (they see all three points) free, the other poses and the principal points constant, every point free."""
    pose_const = np.ones(18, np.uint8); pose_const[[1, 2]] = 0
    return pose_const, np.zeros(18, np.uint8), np.full(2, 0b0110, np.uint16), np.zeros(3, np.uint8)


# ---- one function per entry point: the outputs as numpy arrays ------------------------------------------------------------------------
def run_interpolate(ctx, st, channels):
    from pixsfm_amd.engine import interpolate
    scene = _scene(channels)
    kp = scene["centers"][:8] + np.linspace(-1.3, 1.4, 16).reshape(8, 2)
    return interpolate(ctx, _arena(ctx, scene, st), _cfg(channels), kp, np.arange(8), jacobian=True)


def run_nearest(ctx, st, channels):
    from pixsfm_amd.engine import nearest_references
    scene = _scene(channels)
    kp = scene["centers"][:8] + np.linspace(-1.3, 1.4, 16).reshape(8, 2)
    cand = np.random.default_rng(channels).normal(0, 0.3, (12, channels))
    return nearest_references(ctx, _arena(ctx, scene, st), _cfg(channels), kp, np.arange(8), [0, 2, 3, 5, 6, 8, 9, 11, 12], cand,
                              want_desc=True)


def run_references(ctx, st, channels):
    _, ba = _ba(ctx, st, channels)
    chosen, mean = ba.compute_references(_cfg(channels), _loss(), iters=10, keep_mean=True)
    return chosen, mean, ba.d["refs"].download()


def run_costmap(ctx, st, channels, ot, grad, ps=PS):
    _, ba = _ba(ctx, st, channels, ps)
    return (ba.extract_costmaps(_loss(), as_gradientfield=grad, dtype=ot).download()[0],)


def run_costmap_ex(ctx, st, channels, ot, float_simd):
    _, ba = _ba(ctx, st, channels)
    cm = ba.extract_costmaps(_loss(), dtype=ot, upsampling_factor=2.0, compute_cross_derivative=True,
                             cfg=_cfg(channels, use_float_simd=float_simd))
    assert (cm.H, cm.W, cm.C) == (2 * PS, 2 * PS, 4)
    return (cm.download()[0],)


def _fmap(src, channels):
    return _grid(np.random.default_rng(5).uniform(-1, 1, (channels, 20, 24))).astype(src)


EX_KPS = np.array([[0.3, 0.4], [95.8, 79.9], [48.0, 40.0], [48.37, 5.0], [3.0, 39.51], [60.0, 50.0]])
EX_SIZE = (96.0, 80.0)


def run_extract(ctx, src, dst, channels):
    import torch
    from pixsfm_amd.engine import PatchArena
    arena = PatchArena(ctx, len(EX_KPS), PS, PS, channels, dst)
    arena.extract(0, torch.from_numpy(_fmap(src, channels)).cuda(), EX_KPS, EX_SIZE, l2_normalize=False)
    return arena.download()


@functools.lru_cache(maxsize=None)
def _image(src):
    yy, xx = np.mgrid[0:20, 0:24]
    noise = np.random.default_rng(2).integers(0, 256, (20, 24))
    u8 = np.clip(127 + 90 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + (noise - 127) * 0.3, 0, 255).astype(np.uint8)
    return u8 if src is np.uint8 else u8.astype(F32) / F32(255)


def run_dsift_dense(ctx, src):
    from pixsfm_amd.engine import dsift_dense
    return (dsift_dense(ctx, _image(src)).cpu().numpy()[0],)


def run_dsift_extract(ctx, src, dst):
    from pixsfm_amd.engine import PatchArena
    arena = PatchArena(ctx, len(EX_KPS), PS, PS, 128, dst)
    arena.extract_dsift(0, _image(src), EX_KPS, EX_SIZE)
    return arena.download()


def run_ba_eval(ctx, st, channels, with_jac, float_simd):
    _, ba = _ba(ctx, st, channels)
    out = ba.eval(_cfg(channels, use_float_simd=float_simd), with_jacobian=with_jac, materialize=True)
    return tuple(a.download() for a in out if a is not None)


def run_gram(ctx, st, channels):
    _, ba = _ba(ctx, st, channels)
    rec, built = ba.eval_gram(_cfg(channels), reset=True)
    assert built == ba.n_obs                      # k_gram_build made every matrix
    return (rec.download(),)


def _solve(ctx, ba, gauge, cfg, packed):
    """Two LM iterations with inner iterations; packed: PXR_INNER_PACKED=1 (lists == nullptr) on the exact-order evaluation."""
    from pixsfm_amd.engine import lm_options
    before = os.environ.get("PXR_INNER_PACKED"), ctx.gram_cache
    try:
        if packed:
            os.environ["PXR_INNER_PACKED"] = "1"
            ctx.gram_cache = False
        s = ba.solve(cfg, _loss(), *gauge,
                     options=lm_options(max_iterations=2, use_inner_iterations=True))
    finally:
        os.environ.pop("PXR_INNER_PACKED", None)
        if before[0] is not None:
            os.environ["PXR_INNER_PACKED"] = before[0]
        ctx.gram_cache = before[1]
    summary = np.array([s["iterations"], s["num_successful"], s["initial_cost"], s["final_cost"]])
    return (summary,) + tuple(ba.params())


def run_inner(ctx, st, channels, float_simd, packed):
    scene, ba = _ba(ctx, st, channels)
    return _solve(ctx, ba, _gauge(scene), _cfg(channels, use_float_simd=float_simd), packed)


@functools.lru_cache(maxsize=None)
def _costmaps(ctx, channels):
    """The fp64 cost maps of the 128-channel scene (3 channels: the gradient field; 1: the cost), rounded to fp16 values."""
    return run_costmap(ctx, F64, 128, F64, channels == 3)[0].astype(F16).astype(F64)


def run_inner_costmaps(ctx, st, channels, float_simd):
    from pixsfm_amd.engine import PatchArena
    scene, ba = _ba(ctx, F64, 128)
    cm = PatchArena.from_numpy(ctx, _costmaps(ctx, channels).astype(st), scene["corners"], scene["scales"])
    return _solve(ctx, ba.costmap_problem(cm), _gauge(scene), _cfg(channels, use_float_simd=float_simd), False)


@functools.lru_cache(maxsize=None)
def _ka_scene(channels):
    from pixsfm_amd import synthetic_ka
    p = synthetic_ka.make_ka_problem(n_tracks=2, track_len=3, channels=max(channels, 3), patch_size=PS, seed=4, dtype=F64, sigma=0.4)
    p["patches"] = _grid(p["patches"][..., :channels])
    return p


def _ka(ctx, st, channels):
    from pixsfm_amd.ka_engine import KAProblem
    scene = _ka_scene(channels)
    return KAProblem(ctx, _arena(ctx, scene, st), scene)


def run_ka_eval(ctx, st, channels):
    return tuple(a.download() for a in _ka(ctx, st, channels).eval(_cfg(channels), _loss(), materialize=True))


def run_ka_solve(ctx, st, channels, det):
    ka, before = _ka(ctx, st, channels), ctx.deterministic
    try:
        ctx.deterministic = det
        s, _ = ka.solve(_cfg(channels), _loss(), bound=4.0)
    finally:
        ctx.deterministic = before
    return np.array([s["iterations"], s["num_successful"], s["initial_cost"], s["final_cost"]]), ka.keypoints()


# ---- the matrix: what each site's for_storage / for_channels / for_flag calls enumerate ------------------------------------------
def _matrix():
    m = []
    for st in STORAGES:
        for c in (128, 64, 3, 1):
            m += [(run_interpolate, (st, c)), (run_nearest, (st, c)), (run_references, (st, c))]
            m += [(run_costmap, (st, c, ot, grad)) for ot in STORAGES for grad in (True, False)]
            m += [(run_ba_eval, (st, c, wj, fs)) for wj in (True, False) for fs in ((True, False) if c >= 64 else (False,))]
        for c in (128, 64):
            m += [(run_costmap_ex, (st, c, ot, fs)) for ot in STORAGES for fs in (True, False)]
            m += [(run_inner, (st, c, fs, False)) for fs in (True, False)]           # f16 / f32: Gram-packed + long-track packed
        for c in (3, 1):
            m += [(run_inner_costmaps, (st, c, fs)) for fs in (True, False)]
        for c in (128, 64, 1):
            m += [(run_ka_eval, (st, c))] + [(run_ka_solve, (st, c, det)) for det in (True, False)]
    # launch_costmap_f16: the H == 16 branch, and the generic kernel behind it (a side that is neither 16 nor 8)
    m += [(run_costmap, (F16, 128, ot, grad, ps)) for ot in STORAGES for grad in (True, False) for ps in (16, 6)]
    for st in (F16, F32):
        for c in (128, 64):
            m += [(run_gram, (st, c))] + [(run_inner, (st, c, fs, True)) for fs in (True, False)]   # lists == nullptr
    for src in (F32, F16):
        m += [(run_extract, (src, dst, c)) for dst in STORAGES for c in (128, 64, 3, 1)]
    for src in (np.uint8, F32):
        m += [(run_dsift_dense, (src,))] + [(run_dsift_extract, (src, dst)) for dst in STORAGES]
    return m


def _id(case):
    fn, args = case
    return fn.__name__[4:] + "-" + "-".join(NAME.get(a, str(a)) if isinstance(a, type) else str(int(a)) for a in args)


MATRIX = _matrix()
FP32_PASS_ENTRIES = (run_interpolate, run_nearest, run_references, run_ba_eval, run_ka_eval, run_ka_solve)
_cache = {}


def _run(ctx, fn, args):
    """Every combination runs once per session: the fp64 ones are the others' references."""
    key = (fn.__name__, args)
    if key not in _cache:
        _cache[key] = tuple(np.asarray(a) for a in fn(ctx, *args))
    return _cache[key]


# ---- the checks: each entry point's own tolerances ------------------------------------------------------------------------------------
def _ulps(a, b):   # tests/test_costmap_gpu.py
    it = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    sign = np.int64(1) << (8 * a.dtype.itemsize - 1)
    return np.abs(np.where(ia < 0, -(ia + sign), ia) - np.where(ib < 0, -(ib + sign), ib))


def _stored(a, ot):
    """store_cast of csrc/pxr_costmap.hip: half storage goes through float."""
    return a.astype(F32).astype(F16) if ot is F16 else a.astype(ot)


def _fp64_args(fn, args):
    """The same call on fp64 storage (and fp64 output): the reference of a combination."""
    if fn in (run_costmap, run_costmap_ex):
        return (F64, args[1], F64) + args[3:]
    if fn is run_inner:
        return (F64, args[1], args[2], False)        # fp64 arenas: k_inner_points whatever PXR_INNER_PACKED says
    return (F64,) + args[1:]


def _check(ctx, fn, args):
    from conftest import FP32_PASS_RECORD_ATOL
    got = _run(ctx, fn, args)
    print(_id((fn, args)), " ".join("%s%s" % (a.dtype, list(a.shape)) for a in got))
    if fn is run_extract:              # test_extract_gpu.py: the plain gather is bit exact
        import pxo_extract
        want, corners, scale = pxo_extract.sparse_patches(_fmap(args[0], args[2]), EX_KPS, EX_SIZE, ps=PS, l2_normalize=False, dtype=args[1])
        assert got[0].dtype == want.dtype and np.array_equal(got[0], want)
        assert np.array_equal(got[1], corners) and np.array_equal(got[2], np.tile(scale, (len(EX_KPS), 1)))
        return
    if fn is run_dsift_dense:          # test_dsift_gpu.py
        want = dsift_ref.dsift_numpy(_image(F32).astype(F64), 4, True)
        g = got[0].astype(F64)
        err, err_sq = np.abs(g - want).max(), np.abs(g * g - want * want).max()
        print("  max abs err %.2e, of the squares %.2e" % (err, err_sq))
        assert got[0].shape == want.shape and err_sq <= DENSE_ATOL and err <= ROOTSIFT_ATOL
        return
    if fn is run_dsift_extract:        # test_dsift_gpu.py: the fused producer equals dense -> pxr_arena_extract bit for bit
        import torch
        from pixsfm_amd.engine import PatchArena
        ref = PatchArena(ctx, len(EX_KPS), PS, PS, 128, args[1])
        ref.extract(0, torch.from_numpy(_run(ctx, run_dsift_dense, (args[0],))[0][None]).cuda(), EX_KPS, EX_SIZE)
        for a, b in zip(got, ref.download()):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        return
    if fn is run_gram:                 # test_gram_cache_gpu.py, against pxr_ba_eval on the fp64 arena
        exact = _run(ctx, run_ba_eval, (F64, args[1], True, False))[0]
        print("  max record difference %.2e" % np.abs(got[0][:, :6] - exact[:, :6]).max())
        assert np.array_equal(got[0][:, 6:], exact[:, 6:])
        assert np.abs(got[0][:, :6] - exact[:, :6]).max() < FP32_PASS_RECORD_ATOL
        return
    # The descriptor kernels of fp16 / fp32 storage run the reference's fp32 horizontal pass, the fp64 ones run it in fp64
    # (conftest.py, "the two arithmetics"): against fp64 their outputs are held to conftest's price of that pass, and the fp16
    # arena also to the fp32 arena (the same arithmetic on the same values) at the entry point's own tolerances.
    fp32_pass = fn in FP32_PASS_ENTRIES and args[0] is not F64 and args[1] >= 64
    _compare(fn, args, got, _run(ctx, fn, _fp64_args(fn, args)), fp32_pass)
    if fp32_pass and args[0] is F16:
        _compare(fn, args, got, _run(ctx, fn, (F32,) + args[1:]), False)


def _close(got, want, tol, fp32_pass, rel=False):
    """Within one arithmetic: tol, of max(1, |want|) or (rel) of |want|; across the fp32 pass: FP32_PASS_RECORD_ATOL of max(1, |want|)."""
    from conftest import FP32_PASS_RECORD_ATOL
    err = np.abs(got - want).max() / (max(np.abs(want).max(), 1e-300) if rel and not fp32_pass else max(1.0, np.abs(want).max()))
    print("  %s%s: %.2e" % (got.dtype, list(got.shape), err))
    return got.shape == want.shape and err < (FP32_PASS_RECORD_ATOL if fp32_pass else tol)


def _compare(fn, args, got, want, fp32_pass):
    from conftest import (FP32_PASS_COST_RTOL, FP32_PASS_FINAL_COST_RTOL, FP32_PASS_INNER_FINAL_COST_RTOL, FP32_PASS_PARAM_RTOL)
    assert len(got) == len(want)
    if fn is run_interpolate:          # test_refs_gpu.py
        assert _close(got[0], want[0], 1e-12, fp32_pass) and _close(got[1], want[1], 1e-9, fp32_pass)
    elif fn is run_nearest:            # test_refs_gpu.py
        assert np.array_equal(got[0], want[0]) and (got[0] >= 0).all() and np.array_equal(got[2], want[2])
        assert _close(got[1], want[1], 1e-12, fp32_pass)
    elif fn is run_references:         # test_refs_gpu.py
        assert np.array_equal(got[0], want[0]) and (got[0] >= 0).all()
        assert _close(got[1], want[1], 1e-10, fp32_pass) and _close(got[2], want[2], 1e-10, fp32_pass)
    elif fn is run_costmap:            # test_costmap_gpu.py _check_maps
        g, w = got[0], _stored(want[0], args[2])
        assert g.dtype == w.dtype and g.shape == w.shape
        if g.dtype == F64:
            assert np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
        else:
            d = _ulps(g, w)
            print("  max ulps %d, entries that differ %.2e" % (d.max(), (d > 0).mean()))
            assert d.max() <= 1 and (d > 0).mean() < (1e-3 if g.dtype == F16 else 2e-3)
    elif fn is run_costmap_ex:         # test_costmap_gpu.py test_interpolated_costmaps_match_oracle (fp64 maps: _check_maps' 1e-12)
        g, w = got[0].astype(F64), _stored(want[0], args[2]).astype(F64)
        assert got[0].dtype == args[2] and g.shape == w.shape
        err = (np.abs(g - w) / (np.abs(w).max(axis=(1, 2), keepdims=True) + 1e-30)).max()
        print("  max error relative to the channel's range %.2e" % err)
        assert err < {2: 2e-3, 4: 1e-6, 8: 1e-12}[got[0].dtype.itemsize]
    elif fn is run_ba_eval:            # test_ba_eval_gpu.py TOL; the projection (rec[:, 6:]) is the same code in every storage
        assert _close(got[0][:, 6:], want[0][:, 6:], 1e-10, False, True) and _close(got[0][:, :6], want[0][:, :6], 1e-10, fp32_pass, True)
        assert all(_close(g, w, 1e-10, fp32_pass, True) for g, w in zip(got[1:], want[1:]))
    elif fn in (run_inner, run_inner_costmaps):   # test_ba_inner_gpu.py
        cost_tol = 1e-4 if (fn is run_inner_costmaps or args[3]) else FP32_PASS_INNER_FINAL_COST_RTOL
        print("  final cost %.9e against %.9e, parameters within %.2e" % (got[0][3], want[0][3], max(np.abs(g - w).max() for g, w in zip(got[1:], want[1:]))))
        assert np.array_equal(got[0][:2], want[0][:2]) and got[0][1] >= 1
        assert abs(got[0][3] - want[0][3]) < cost_tol * max(want[0][3], 1e-9)
        assert all(np.abs(g - w).max() < 1e-4 for g, w in zip(got[1:], want[1:]))
    elif fn is run_ka_eval:            # test_ka_gpu.py
        assert all(_close(g, w, 1e-10, fp32_pass, True) for g, w in zip(got, want))
    elif fn is run_ka_solve:           # test_ka_gpu.py; across the fp32 pass conftest's cost and parameter tolerances
        cost0, cost1, kp = (FP32_PASS_COST_RTOL, FP32_PASS_FINAL_COST_RTOL, FP32_PASS_PARAM_RTOL * np.abs(want[1]).max()) if fp32_pass else (1e-10, 1e-7, 1e-6)
        print("  costs %.3e %.3e, keypoints %.2e" % (abs(got[0][2] / want[0][2] - 1), abs(got[0][3] - want[0][3]) / max(want[0][3], 1e-6), np.abs(got[1] - want[1]).max()))
        assert np.array_equal(got[0][:2], want[0][:2])
        assert abs(got[0][2] - want[0][2]) < cost0 * want[0][2] and abs(got[0][3] - want[0][3]) < cost1 * max(want[0][3], 1e-6)
        assert np.abs(got[1] - want[1]).max() < kp
    else:
        raise AssertionError("no check for %s" % fn.__name__)


@pytest.mark.parametrize("case", MATRIX, ids=_id)
def test_combination_launches_its_kernel(ctx, case):
    _check(ctx, *case)


# ---- per site: an arena it does not support ------------------------------------------------------------------------------------------
def _unsupported(ctx):
    """(site, status code the site has always returned, call) -- 32 channels, or a source type without a kernel."""
    import torch
    from pixsfm_amd import _lib
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, interpolate, nearest_references
    from pixsfm_amd.ka_engine import KAProblem
    EINVAL, EUNSUPPORTED = -1, _lib.PXR_EUNSUPPORTED
    scene = dict(_scene(64))
    scene["patches"], scene["refs"] = scene["patches"][..., :32], scene["refs"][:, :32]
    a32 = _arena(ctx, scene, F16)
    ba = BAProblem(ctx, a32, scene)
    kp, idx = scene["centers"][:4], np.arange(4)
    ka_scene = dict(_ka_scene(64))
    ka_scene["patches"] = ka_scene["patches"][..., :32]
    ka = KAProblem(ctx, _arena(ctx, ka_scene, F16), ka_scene)
    fmap64 = torch.zeros((32, 20, 24), dtype=torch.float64).cuda()
    f16_image = torch.zeros((20, 24), dtype=torch.float16).cuda()

    def extract_f64_source():
        arena = PatchArena(ctx, 1, PS, PS, 64, F16)
        _lib.check(ctx.lib.pxr_arena_extract(ctx.handle, arena.handle, 0, 1, fmap64.data_ptr(), _lib.F64, 20, 24,
                                             ctx.to_device(EX_KPS[:1], F64).ptr, 96.0, 80.0, 0), "pxr_arena_extract")

    def dsift_f16_image():
        out = torch.empty((128, 20, 24), dtype=torch.float32).cuda()
        _lib.check(ctx.lib.pxr_dsift_dense(ctx.handle, f16_image.data_ptr(), _lib.F16, 20, 24, 4, 1, 0.2, out.data_ptr()), "pxr_dsift_dense")

    return [
        ("pxr_interpolate", EUNSUPPORTED, lambda: interpolate(ctx, a32, interp_cfg(), kp, idx)),
        ("pxr_nearest_references", EUNSUPPORTED, lambda: nearest_references(ctx, a32, interp_cfg(), kp, idx, [0, 1, 2, 3, 4], np.zeros((4, 32)))),
        ("pxr_ba_compute_references", EINVAL, lambda: ba.compute_references(interp_cfg(), _loss())),
        ("pxr_costmap_extract", EUNSUPPORTED, lambda: ba.extract_costmaps(_loss())),
        ("pxr_costmap_extract_ex", EUNSUPPORTED, lambda: ba.extract_costmaps(_loss(), upsampling_factor=2.0)),
        ("pxr_costmap_extract_ex, 3 channels", EUNSUPPORTED, lambda: _ba(ctx, F16, 3)[1].extract_costmaps(_loss(), upsampling_factor=2.0)),
        ("pxr_arena_extract", EUNSUPPORTED, lambda: a32.extract(0, fmap64.float(), EX_KPS[:1], EX_SIZE)),
        ("pxr_arena_extract, fp64 source", EUNSUPPORTED, extract_f64_source),
        ("pxr_dsift_extract", EUNSUPPORTED, lambda: a32.extract_dsift(0, _image(np.uint8), EX_KPS[:1], EX_SIZE)),
        ("pxr_dsift_dense, fp16 image", EUNSUPPORTED, dsift_f16_image),
        ("pxr_ba_eval", EUNSUPPORTED, lambda: ba.eval(interp_cfg())),
        ("pxr_ba_eval_gram", EINVAL, lambda: ba.eval_gram(interp_cfg())),
        ("pxr_ba_solve, inner iterations", EUNSUPPORTED, lambda: _solve(ctx, ba, _gauge(scene), interp_cfg(), False)),
        ("pxr_ka_eval", EUNSUPPORTED, lambda: ka.eval(interp_cfg(), _loss())),
        ("pxr_ka_solve", EUNSUPPORTED, lambda: ka.solve(interp_cfg(), _loss())),
    ]


def _refusal(call):
    from pixsfm_amd import PixsfmHipError
    try:
        call()
    except PixsfmHipError as e:
        return e.code, str(e).split("): ", 1)[-1]
    return 0, ""


def test_unsupported_arenas_are_refused_as_before(ctx):
    for site, code, call in _unsupported(ctx):
        got, message = _refusal(call)
        print(site, got, message)
        assert got == code and message not in ("", "?"), site


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(ROOT, "pixel-perfect-sfm_amd"), os.path.join(ROOT, "oracle")]
    from pixsfm_amd.engine import Context
    context = Context(0)
    for case_ in MATRIX:
        h = hashlib.sha256()
        for out_ in _run(context, *case_):
            h.update(np.ascontiguousarray(out_).tobytes())
        print(_id(case_), h.hexdigest(), flush=True)
    for site_, _, call_ in _unsupported(context):
        print("refused:", site_, *_refusal(call_), flush=True)
