"""CPU: the dense-SIFT descriptor's two float64 restatements (tests/dsift_ref.py) against each other and against the
descriptor's defining properties, the C-ABI / ctypes surface of the producer, and the host side of FeatureExtractor
(pixsfm/features/extractor.py: resize, grey conversion, configuration checks) -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsift_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (7, 1), (2, 5), (17, 23), (31, 18)]


@pytest.mark.parametrize("s", [2, 4, 6, 8])
@pytest.mark.parametrize("rootsift", [True, False])
def test_the_two_restatements_agree(s, rootsift):
    rng = np.random.default_rng(s + 10 * rootsift)
    for h, w in SIZES:
        img = rng.random((h, w))
        a = dsift_ref.dsift_numpy(img, s, rootsift)
        b = dsift_ref.dsift_torch(img, s, rootsift)
        assert a.shape == b.shape == (128, h, w)
        assert np.abs(a - b).max() < 1e-12, (h, w, s, rootsift)


def test_pooling_kernel():
    assert np.allclose(dsift_ref.pool_kernel(4), [0.25, 0.75, 0.75, 0.25])
    for s in (2, 4, 6, 8):
        k = dsift_ref.pool_kernel(s)
        assert np.allclose(k, k[::-1]) and abs(k.sum() - s / 2) < 1e-12


@pytest.mark.parametrize("s", [2, 4, 6, 8])
def test_defining_properties(s):
    rng = np.random.default_rng(100 + s)
    img = rng.random((19, 26))
    d = dsift_ref.dsift_numpy(img, s, rootsift=True)
    assert np.abs(np.sqrt((d * d).sum(0)) - 1.0).max() < 1e-8          # the L1 step makes the square roots unit-L2
    assert d.min() >= 0.0 and d.max() <= 1.0
    d = dsift_ref.dsift_numpy(img, s, rootsift=False, clipval=0.2)
    assert d.min() >= 0.0 and d.max() <= 1.0
    assert np.abs(np.sqrt((d * d).sum(0)) - 1.0).max() < 1e-12


@pytest.mark.parametrize("s", [2, 4, 6, 8])
@pytest.mark.parametrize("rootsift", [True, False])
def test_horizontal_flip_equivariance(s, rootsift):
    """D(fliplr I)[a, sy, sx](y, x) = D(I)[(4 - a) mod 8, sy, 3 - sx](y, w - 1 - x), borders included: checks the index
    conventions of the pooling and the spatial gather independently of how they were written."""
    rng = np.random.default_rng(7 * s + rootsift)
    for h, w in ((13, 17), (6, 2), (21, 9)):
        img = rng.random((h, w))
        d = dsift_ref.dsift_numpy(img, s, rootsift).reshape(8, 4, 4, h, w)
        f = dsift_ref.dsift_numpy(img[:, ::-1], s, rootsift).reshape(8, 4, 4, h, w)
        want = d[[(4 - a) % 8 for a in range(8)]][:, :, ::-1, :, ::-1]
        assert np.abs(f - want).max() < 1e-8, (h, w)


def test_grey_conversion_is_pil_convert_L_over_255():
    from PIL import Image
    from pixsfm_amd.api import FeatureExtractor
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    ex = FeatureExtractor({"model": {"name": "dsift"}, "max_edge": 4000})
    levels, size = ex.preprocess(rgb)
    want = np.asarray(Image.fromarray(rgb).convert("L"))
    assert size == (31, 23) and len(levels) == 1
    assert levels[0].dtype == np.uint8 and np.array_equal(levels[0], want)
    u8, f = dsift_ref.grey_of(rgb)
    assert np.array_equal(u8, want) and f.dtype == np.float32 and np.array_equal(f, want.astype(np.float32) / np.float32(255))
    # the `image` model: RGB / 255, channels first; grayscale: one channel
    img = FeatureExtractor({"model": {"name": "image"}, "max_edge": 4000}).preprocess(rgb)[0][0]
    assert img.shape == (3, 23, 31) and np.array_equal(img, rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    g = FeatureExtractor({"model": {"name": "image", "grayscale": True}, "max_edge": 4000}).preprocess(rgb)[0][0]
    assert g.shape == (1, 23, 31)


def test_scaled_image_size_and_resize_follow_the_reference():
    from PIL import Image
    from pixsfm_amd.api import FeatureExtractor
    ex = FeatureExtractor({"model": {"name": "dsift"}, "max_edge": 100, "pyr_scales": [1.0, 0.5], "resize": "BILINEAR"})
    for w, h in ((300, 200), (99, 40), (101, 101), (37, 250)):
        im = Image.new("RGB", (w, h))
        for p in (1.0, 0.5):
            want = [int(round(min(100 / max(w, h), 1) * x * p)) for x in [w, h]]     # extractor.py get_scaled_image_size
            assert ex.get_scaled_image_size(im, p) == want
    rgb = np.random.default_rng(2).integers(0, 256, (200, 300, 3), dtype=np.uint8)
    levels, size = ex.preprocess(rgb)
    assert size == (300, 200) and [lv.shape for lv in levels] == [(67, 100), (33, 50)]
    want = np.asarray(Image.fromarray(rgb).resize((100, 67), Image.BILINEAR).convert("L"))
    assert np.array_equal(levels[0], want)
    assert ex.channels_per_level == [128, 128]


def test_configuration_checks():
    from pixsfm_amd.api import FeatureExtractor
    for name in ("s2dnet", "vggnet"):
        with pytest.raises(ValueError, match="weights"):
            FeatureExtractor({"model": {"name": name}})
    with pytest.raises(ValueError, match="weights"):
        FeatureExtractor()                                   # the reference's default model is s2dnet
    bad = [{"model": {"name": "sift"}},
           {"model": {"name": "dsift", "num_ang_bins": 4}},
           {"model": {"name": "dsift", "num_spatial_bins": 2}},
           {"model": {"name": "dsift", "spatial_bin_size": 3}},
           {"model": {"name": "dsift", "spatial_bin_size": 10}},
           {"model": {"name": "dsift", "spatial_bin_size": 0}},
           {"model": {"name": "dsift", "unknown": 1}},
           {"model": {"name": "dsift"}, "use_cache": True},
           {"model": {"name": "dsift"}, "device": "cpu"},
           {"model": {"name": "dsift"}, "device": "tpu"},
           {"model": {"name": "dsift"}, "dtype": "int8"},
           {"model": {"name": "dsift"}, "patch_size": 17},
           {"model": {"name": "dsift"}, "resize": "NEAREST"}]
    for conf in bad:
        with pytest.raises(ValueError):
            FeatureExtractor(conf)
    for dev in ("auto", "cuda", "cuda:0"):
        ex = FeatureExtractor({"model": {"name": "dsift", "spatial_bin_size": 6, "rootsift": False}, "device": dev})
        assert ex.conf["model"]["clipval"] == 0.2 and ex.conf["model"]["spatial_bin_size"] == 6
    assert FeatureExtractor({"model": {"name": "image", "grayscale": True}}).channels_per_level == [1]


def test_sparse_extraction_needs_keypoints():
    from pixsfm_amd.api import FeatureExtractor, features_from_image_list
    ex = FeatureExtractor({"model": {"name": "dsift"}})
    with pytest.raises(AttributeError):
        features_from_image_list(ex, "/nonexistent", ["a.png"])
    with pytest.raises(RuntimeError):
        ex.tensor_to_fmap(np.zeros((32, 32), np.uint8), (32, 32), None)
    with pytest.raises(ValueError):
        ex.tensor_to_fmap(np.zeros((32, 32), np.uint8), (32, 32), np.zeros((3, 2)), keypoint_ids=[1, 2])


def test_matched_keypoints_of_a_graph():
    from pixsfm_amd.api import extract_patchdata_from_graph
    from pixsfm_amd.api.base import Graph
    g = Graph()
    for name, k in (("b.jpg", 4), ("a.jpg", 2), ("b.jpg", 1), ("a.jpg", 9)):
        g.find_or_create_node(name, k)
    assert extract_patchdata_from_graph(g) == {"b.jpg": [4, 1], "a.jpg": [2, 9]}


def test_c_abi_declares_the_producer():
    from pixsfm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pixsfm_hip.h")).read()
    assert "PXR_U8 = 3" in hdr and _lib.U8 == 3
    for name in ("pxr_dsift_dense", "pxr_dsift_extract"):
        assert name + "(" in hdr and name in _lib.declared_symbols()
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "pxr_dsift_dense") and hasattr(lib, "pxr_dsift_extract")


def test_product_does_not_use_the_test_oracle():
    pkg = os.path.join(ROOT, "pixel-perfect-sfm_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                assert "dsift_ref" not in open(os.path.join(dp, f)).read(), f


def test_no_gpu_means_a_loud_failure():
    import torch
    from pixsfm_amd import PixsfmHipError
    from pixsfm_amd.api import FeatureExtractor
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ex = FeatureExtractor({"model": {"name": "dsift"}})
    with pytest.raises(PixsfmHipError):
        ex(np.zeros((40, 40), np.uint8), np.array([[20.0, 20.0]]))
