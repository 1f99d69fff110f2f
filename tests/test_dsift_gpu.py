"""GPU: the dense-SIFT producer (csrc/pxr_dsift.hip) through the C-ABI and the extraction API.
  * pxr_dsift_dense against the float64 restatement (tests/dsift_ref.py) of the descriptor defined in DESIGN.md §16;
  * the fused pxr_dsift_extract equals pxr_dsift_dense followed by pxr_arena_extract BIT FOR BIT (patches, corners, scales);
  * FeatureExtractor on a PNG equals the host pipeline (PIL -> dsift_ref -> L2 -> fp16 -> gather) in both branches;
  * photographs -> GPU dense SIFT -> arena -> featuremetric KA / BA on real texture (tests/real_scene.py).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsift_ref  # noqa: E402

pytestmark = pytest.mark.gpu
# Measured on an MI355X against the float64 definition (the issue's first estimate was 1e-5 for everything):
#   rootsift off: <= 6.5e-7 over every size, input type and s -> held at 1e-6;
#   rootsift on: up to 3.0e-4.  The fp32 angle binning puts ~1e-7 of a pixel's magnitude into a neighbouring bin where the exact
#   angle sits on a bin boundary (gy == 0 with gx < 0: atan2 = pi rounded, o = 12 +- 1 ulp; frequent in uint8 images), and
#   rootsift's sqrt(x + 1e-10) turns an absolute 1e-7 next to zero into 3e-4.  The reference model runs the same fp32
#   arithmetic.  So the rootsift output is held at 1e-6 in its SQUARE (n / |n|_1 + 1e-10, where errors stay linear) and at
#   5e-4 directly.
DENSE_ATOL = 1e-6
ROOTSIFT_ATOL = 5e-4


def _ulp16(a, b):
    return np.abs(a.view(np.int16).astype(np.int32) - b.view(np.int16).astype(np.int32))


def _image(rng, h, w, dtype):
    u8 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    # smooth structure + noise: real gradients of every orientation, a few flat patches
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
    u8 = np.clip(base + (u8.astype(np.float64) - 127) * 0.3, 0, 255).astype(np.uint8)
    u8[: h // 4, : w // 4] = 77
    if dtype == "u8":
        return u8, u8.astype(np.float32) / np.float32(255)
    f = (u8.astype(np.float32) / np.float32(255) + rng.normal(0, 0.01, (h, w)).astype(np.float32)).astype(np.float32)
    return f, f


def _dense_error(got, want, rootsift):
    """(max abs error, max abs error of the squares): the latter is the check of a rootsift output."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    return np.abs(got - want).max(), (np.abs(got * got - want * want).max() if rootsift else np.abs(got - want).max())


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("s", [2, 4, 6, 8])
@pytest.mark.parametrize("rootsift", [True, False])
def test_dense_kernel_equals_the_float64_definition(ctx, dtype, s, rootsift):
    from pixsfm_amd.engine import dsift_dense
    rng = np.random.default_rng(s + 7 * rootsift + (dtype == "f32"))
    worst, worst_sq = 0.0, 0.0
    for h, w in ((17, 17), (40, 33), (77, 123)):
        img, grey = _image(rng, h, w, dtype)
        got = dsift_dense(ctx, img, spatial_bin_size=s, rootsift=rootsift).cpu().numpy()
        want = dsift_ref.dsift_numpy(grey.astype(np.float64), s, rootsift)
        assert got.shape == (1, 128, h, w)
        e, e2 = _dense_error(got[0], want, rootsift)
        worst, worst_sq = max(worst, e), max(worst_sq, e2)
    print("dense max abs err (dtype %s, s %d, rootsift %d): %.2e, of the squares %.2e" % (dtype, s, rootsift, worst, worst_sq))
    assert worst_sq <= DENSE_ATOL and worst <= (ROOTSIFT_ATOL if rootsift else DENSE_ATOL)


def test_dense_kernel_at_full_size(ctx):
    import torch
    from pixsfm_amd.engine import dsift_dense
    rng = np.random.default_rng(5)
    img, grey = _image(rng, 1200, 1600, "u8")
    got = dsift_dense(ctx, torch.from_numpy(img).cuda()).cpu().numpy()[0]      # a device tensor as input
    want = dsift_ref.dsift_numpy(grey.astype(np.float64), 4, True)
    err, err_sq = _dense_error(got, want, True)
    print("dense max abs err 1200 x 1600: %.2e, of the squares %.2e" % (err, err_sq))
    assert err_sq <= DENSE_ATOL and err <= ROOTSIFT_ATOL


def _keypoints(rng, n, w, h, image_w, image_h):
    """Keypoints in ORIGINAL image coordinates: inside, on, near and outside every border, plus corners."""
    kp = rng.uniform([0, 0], [image_w, image_h], (n, 2))
    edge = np.array([[0, 0], [image_w, image_h], [-5, 3], [image_w + 9, 0.5 * image_h], [0.5 * image_w, -30],
                     [0.3 * image_w, image_h + 1e3], [1, 1], [image_w - 1, image_h - 1], [2.5, 0.5 * image_h],
                     [0.5 * image_w, image_h - 3.2], [-1e9, 1e9], [np.nan, 4.0]])
    return np.concatenate([kp, edge])


@pytest.mark.parametrize("arena_dtype", [np.float16, np.float32])
@pytest.mark.parametrize("ps", [8, 10, 16])
def test_fused_producer_equals_dense_then_extract_bit_for_bit(ctx, arena_dtype, ps):
    from pixsfm_amd.engine import PatchArena, dsift_dense
    rng = np.random.default_rng(ps)
    for (h, w, image_w, image_h), dtype, s, rootsift, l2 in (((61, 90, 90.0, 61.0), "u8", 4, True, True),
                                                           ((37, 29, 74.0, 58.0), "f32", 8, False, True),
                                                           ((ps + 1, ps + 3, 3.0 * (ps + 3), 3.0 * (ps + 1)), "u8", 2, True, False),
                                                           ((150, 111, 111.0, 150.0), "f32", 6, True, True)):
        img, _ = _image(rng, h, w, dtype)
        kp = _keypoints(rng, 300, w, h, image_w, image_h)
        n = len(kp)
        fused = PatchArena(ctx, n + 3, ps, ps, 128, arena_dtype)
        assert fused.extract_dsift(3, img, kp, (image_w, image_h), spatial_bin_size=s, rootsift=rootsift,
                                   l2_normalize=l2) == n
        dense = dsift_dense(ctx, img, spatial_bin_size=s, rootsift=rootsift)
        ref = PatchArena(ctx, n + 3, ps, ps, 128, arena_dtype)
        ref.extract(3, dense, kp, (image_w, image_h), l2_normalize=l2)
        fp, fc, fs = fused.download(3)
        rp, rc, rs = ref.download(3)
        assert np.array_equal(fc, rc) and np.array_equal(fs, rs)
        assert fp.tobytes() == rp.tobytes(), (h, w, dtype, s, rootsift, np.abs(fp.astype(np.float64) - rp).max())
        # and the host restatement of the gather on the same dense map
        want, wc, wsc = dsift_ref.sparse_patches(dense.cpu().numpy()[0], kp[:-1], (image_w, image_h), ps, l2, arena_dtype)
        assert np.array_equal(fc[:-1], wc) and np.allclose(fs[0], wsc)
        fused.close(); ref.close()


def test_invalid_arguments_are_rejected(ctx):
    from pixsfm_amd import PixsfmHipError
    from pixsfm_amd._lib import PXR_EUNSUPPORTED
    from pixsfm_amd.engine import PatchArena, dsift_dense
    img = np.zeros((40, 40), np.uint8)
    kp = np.array([[20.0, 20.0]])
    a64 = PatchArena(ctx, 1, 16, 16, 64, np.float16)
    with pytest.raises(PixsfmHipError) as e:
        a64.extract_dsift(0, img, kp, (40, 40))
    assert e.value.code == PXR_EUNSUPPORTED
    a = PatchArena(ctx, 2, 16, 16, 128, np.float16)
    for s in (3, 10, 0):
        with pytest.raises(PixsfmHipError) as e:
            a.extract_dsift(0, img, kp, (40, 40), spatial_bin_size=s)
        assert e.value.code == PXR_EUNSUPPORTED
        with pytest.raises(PixsfmHipError):
            dsift_dense(ctx, img, spatial_bin_size=s)
    with pytest.raises(PixsfmHipError) as e:
        a.extract_dsift(0, np.zeros((16, 40), np.uint8), kp, (40, 16))          # not larger than the patch
    assert e.value.code == -1
    with pytest.raises(PixsfmHipError):
        a.extract_dsift(1, img, np.zeros((2, 2)), (40, 40))                   # outside the arena
    with pytest.raises(ValueError):
        a.extract_dsift(0, img.astype(np.float16), kp, (40, 40))
    a.close(); a64.close()


def _write_png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)


@pytest.mark.parametrize("overwrite_sparse", [None, False])
def test_feature_extractor_on_a_png_equals_the_host_pipeline(ctx, tmp_path, overwrite_sparse):
    from PIL import Image
    from pixsfm_amd.api import FeatureExtractor
    from pixsfm_amd.api.features import FeatureMap, kDenseId
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:150, 0:200]
    rgb = np.stack([127 + 100 * np.sin(xx / (5.0 + c)) * np.cos(yy / (4.0 + c)) for c in range(3)], -1)
    rgb = np.clip(rgb + rng.normal(0, 12, rgb.shape), 0, 255).astype(np.uint8)
    path = str(tmp_path / "view.png")
    _write_png(path, rgb)
    ex = FeatureExtractor({"model": {"name": "dsift"}, "max_edge": 160, "resize": "BILINEAR"}, ctx=ctx)
    kp = np.concatenate([rng.uniform([0, 0], [200, 150], (40, 2)), [[0, 0], [199.9, 149.9], [-3, 70]]])
    ids = np.arange(len(kp)) * 3 + 1
    out = ex(path, kp, ids, overwrite_sparse=overwrite_sparse)
    assert len(out) == 1
    data = out[0]
    # the host pipeline: PIL resize + convert("L") / 255 -> the descriptor in the reference model's fp32 arithmetic (torch CPU;
    # the float64 definition differs from ANY fp32 run by up to 3e-4 next to zero, see ROOTSIFT_ATOL) -> fp32 L2 -> fp16 -> gather
    grey = np.asarray(Image.open(path).resize((160, 120), Image.BILINEAR).convert("L")).astype(np.float32) / np.float32(255)
    dense = dsift_ref.dsift_torch(grey, dtype=np.float32)
    scale = np.array((160 / 200, 120 / 150))
    assert np.allclose(data["metadata"]["scale"], scale)
    if overwrite_sparse is None:
        want, corners, _ = dsift_ref.sparse_patches(dense, kp, (200, 150), 16)
        assert data["metadata"]["is_sparse"] and list(data["keypoint_ids"]) == list(ids)
        assert np.array_equal(data["corners"], corners) and data["patches"].dtype == np.float16
        d = _ulp16(data["patches"], want)
    else:
        want = dense / np.sqrt((dense.astype(np.float64) ** 2).sum(0)).astype(np.float32)
        want = want.astype(np.float16).transpose(1, 2, 0)[None]
        assert not data["metadata"]["is_sparse"] and list(data["keypoint_ids"]) == [kDenseId]
        assert data["patches"].shape == (1, 120, 160, 128)
        d = _ulp16(data["patches"], want)
    absd = np.abs(data["patches"].astype(np.float64) - want).max()
    print("extractor vs host pipeline: %.5f of the values within 1 fp16 ulp, max %d ulp, max abs %.2e"
          % ((d <= 1).mean(), d.max(), absd))
    # measured: 1e-5 (sparse) / 1e-4 (dense) of the values beyond 1 ulp -- rootsift's fp32 boundary cases (ROOTSIFT_ATOL) -- 1.2e-4 abs
    assert (d <= 1).mean() > 0.9995 and (d == 0).mean() > 0.99 and absd <= ROOTSIFT_ATOL
    fm = ex(path, kp, ids, as_dict=False, overwrite_sparse=overwrite_sparse)[0]
    assert isinstance(fm, FeatureMap) and fm.is_sparse == (overwrite_sparse is None)


def test_image_model_through_the_extractor(ctx, tmp_path):
    from pixsfm_amd.api import FeatureExtractor
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    path = str(tmp_path / "im.png")
    _write_png(path, rgb)
    ex = FeatureExtractor({"model": {"name": "image"}, "l2_normalize": False, "dtype": "float"}, ctx=ctx)
    kp = rng.uniform([0, 0], [80, 60], (5, 2))
    data = ex(path, kp)[0]
    want, corners, _ = dsift_ref.sparse_patches(rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255), kp, (80, 60), 16,
                                                l2_normalize=False, dtype=np.float32)
    assert np.array_equal(data["corners"], corners) and np.array_equal(data["patches"], want)


# ---- photographs -> GPU dense SIFT -> arena -> KA / BA ------------------------------------------------------------------
@pytest.fixture(scope="module")
def dsift_scene(ctx, tmp_path_factory):
    """The rendered views of the reference's demo photographs written as PNGs, their DSIFT patches from
    features_from_image_list(device=True): one arena, views in order, observations of a view in order."""
    import real_scene
    from pixsfm_amd.api import FeatureExtractor, features_from_image_list
    from pixsfm_amd.api.features import ArenaPatch
    scene = real_scene.make_scene(kind="image")
    d = tmp_path_factory.mktemp("views")
    names, kps = [], {}
    for v, view in enumerate(scene["fmaps"]):                      # kind="image": RGB / 255, (3, VIEW, VIEW)
        name = "view%02d.png" % v
        _write_png(str(d / name), np.round(view.transpose(1, 2, 0) * 255).astype(np.uint8))
        names.append(name)
        kps[name] = scene["detected"][scene["obs_image"] == v]
    ex = FeatureExtractor({"model": {"name": "dsift"}, "max_edge": 2000}, ctx=ctx)
    fm = features_from_image_list(ex, str(d), names, keypoints=kps, device=True)
    arena = fm.fset(0).arena
    order = np.argsort(scene["obs_image"], kind="stable")
    inv = np.empty(len(order), np.int64); inv[order] = np.arange(len(order))
    # the FeatureMaps hold handles into the one arena
    for v, name in enumerate(names):
        fmap = fm.fset(0).fmap(name)
        sel = np.nonzero(scene["obs_image"] == v)[0]
        assert sorted(fmap.patches) == list(range(len(sel)))
        assert all(isinstance(p, ArenaPatch) and p.arena is arena and p.index == inv[sel[k]] for k, p in fmap.patches.items())
    return scene, fm, arena, inv, str(d), names, ex


def test_device_features_equal_the_host_extraction(ctx, dsift_scene):
    from pixsfm_amd.api import features_from_image_list
    scene, fm, arena, inv, d, names, ex = dsift_scene
    patches, corners, scales = arena.download()
    assert arena.n == len(inv) and arena.C == 128 and np.allclose(scales, 1.0)
    kps = {name: scene["detected"][scene["obs_image"] == v] for v, name in enumerate(names[:2])}
    host = features_from_image_list(ex, d, names[:2], keypoints=kps)
    for v, name in enumerate(names[:2]):
        sel = np.nonzero(scene["obs_image"] == v)[0]
        hm = host.fset(0).fmap(name)
        for k in range(len(sel)):
            assert np.array_equal(hm.patches[k].data, patches[inv[sel[k]]])


def _truth_error(scene, kp):
    root = scene["node_const"].astype(bool)
    err = np.zeros(len(kp))
    for p in range(len(scene["xyz"])):
        ids = np.nonzero(scene["obs_point"] == p)[0]
        r = ids[root[ids]][0]
        off = scene["detected"][r] - scene["centers"][r]
        err[ids] = np.linalg.norm(kp[ids] - (scene["centers"][ids] + off), axis=1)
    return err[~root]


def test_keypoint_adjustment_on_dsift_of_real_texture(ctx, dsift_scene):
    from pixsfm_amd.engine import interp_cfg, lm_options, make_loss
    from pixsfm_amd.ka_engine import KAProblem
    scene, fm, arena, inv, *_ = dsift_scene
    prob = dict(kp=scene["detected"].copy(), node_patch=inv.astype(np.int64), node_const=scene["node_const"],
                node_problem=scene["node_problem"], edge_src=scene["edge_src"], edge_dst=scene["edge_dst"], edge_w=scene["edge_w"])
    ka = KAProblem(ctx, arena, prob)
    total, _ = ka.solve(interp_cfg(), make_loss("cauchy", [0.25]), bound=4.0, options=lm_options(parameter_tolerance=1e-5),
                        per_problem=True)
    kp = ka.keypoints()
    e0, e1 = _truth_error(scene, scene["detected"]), _truth_error(scene, kp)
    print("DSIFT KA: median truth error %.3f -> %.3f px (x%.3f), cost %.4g -> %.4g"
          % (np.median(e0), np.median(e1), np.median(e1) / np.median(e0), total["initial_cost"], total["final_cost"]))
    assert total["final_cost"] < total["initial_cost"]
    assert np.median(e1) < 0.75 * np.median(e0), (np.median(e0), np.median(e1))
    assert np.abs(kp - scene["detected"]).max() <= 4.0 + 1e-9                   # the box bound: 4 map texels at scale 1


def test_bundle_adjustment_with_dsift_references_lowers_the_cost(ctx, dsift_scene):
    from pixsfm_amd.engine import BAProblem, interp_cfg, lm_options, make_loss
    scene, fm, arena, inv, *_ = dsift_scene
    n_img, n_pts = len(scene["qvec"]), len(scene["xyz"])
    prob = {k: scene[k] for k in ("obs_image", "obs_point", "image_camera", "qvec", "tvec", "cam_model", "cam_params", "xyz")}
    prob["obs_patch"] = inv.astype(np.int64)
    prob["refs"] = np.zeros((n_pts, 128))
    ba = BAProblem(ctx, arena, prob)
    ref_obs, _ = ba.compute_references(interp_cfg(), make_loss("cauchy", [0.25]), iters=100)
    assert (ref_obs >= 0).all()
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    gauge = (pose_const, tmask, np.full(n_img, 0b1111, np.uint16), np.zeros(n_pts, np.uint8))
    s = ba.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge, options=lm_options(max_iterations=6))
    print("DSIFT BA: cost %.5g -> %.5g (x%.3f)" % (s["initial_cost"], s["final_cost"], s["final_cost"] / s["initial_cost"]))
    assert s["final_cost"] < 0.9 * s["initial_cost"]


def test_features_from_reconstruction_and_graph(ctx, dsift_scene):
    from pixsfm_amd.api import extract_patchdata_from_graph, features_from_graph, features_from_reconstruction
    from pixsfm_amd.api.base import Graph
    from pixsfm_amd.api.reconstruction import Camera, Image, Point2D, Point3D, Reconstruction
    scene, fm, arena, inv, d, names, ex = dsift_scene
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_RADIAL", 320, 320, scene["cam_params"][0][:4]))
    for p in range(len(scene["xyz"])):
        rec.add_point3D(p + 1, Point3D(scene["gt_xyz"][p]))
    for v, name in enumerate(names[:3]):
        im = Image(v + 1, name, 1, scene["gt_qvec"][v], scene["gt_tvec"][v])
        im.points2D.append(Point2D((0, 0)))                                 # an unobserved keypoint: id 0 is not extracted
        for i in np.nonzero(scene["obs_image"] == v)[0]:
            im.points2D.append(Point2D(scene["centers"][i], int(scene["obs_point"][i]) + 1))
        rec.add_image(im)
    got = features_from_reconstruction(ex, rec, d, device=True)
    host = features_from_reconstruction(ex, rec, d)
    a = got.fset(0).arena
    patches = a.download()[0]
    for v, name in enumerate(names[:3]):
        n = int((scene["obs_image"] == v).sum())
        g, h = got.fset(0).fmap(name), host.fset(0).fmap(name)
        assert sorted(g.patches) == sorted(h.patches) == list(range(1, n + 1))
        for k in g.patches:
            assert np.array_equal(patches[g.patches[k].index], h.patches[k].data)
    g = Graph()
    for v, name in enumerate(names[:2]):
        for k in (5, 0, 3):
            g.find_or_create_node(name, k)
    kps = {name: scene["detected"][scene["obs_image"] == v] for v, name in enumerate(names[:2])}
    fg = features_from_graph(ex, d, g, keypoints_dict=kps, device=True)
    assert extract_patchdata_from_graph(g) == {names[0]: [5, 0, 3], names[1]: [5, 0, 3]}
    pa = fg.fset(0).arena.download()[0]
    for v, name in enumerate(names[:2]):
        for k, p in fg.fset(0).fmap(name).patches.items():
            q = fm.fset(0).fmap(name).patches[k]
            assert np.array_equal(pa[p.index], q.arena.download(q.index, 1)[0][0])
