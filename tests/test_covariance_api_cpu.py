"""CPU: the Python surface of the covariance estimation -- symbols, indexing by id, units, scaling, the error text."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_symbols_are_exported_and_declared():
    from pixsfm_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("pxr_dense_spd_inverse", "pxr_ba_covariance"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols()
    header = open(os.path.join(ROOT, "include", "pixsfm_hip.h")).read()
    assert re.search(r"int pxr_dense_spd_inverse\(pxr_ctx\* ctx, double\* d_a, int n, int\* h_info\);", header)
    assert "pxr_cov_summary" in header and "HALF-angle" in header
    # the ctypes mirror of pxr_cov_summary: two int32, one int64, three doubles
    assert C.sizeof(_lib.CovSummary) == 4 + 4 + 8 + 3 * 8


def test_column_layout_follows_the_solvers_order():
    from pixsfm_amd.engine import column_layout
    cols = column_layout([1, 0, 0], [0, 0b010, 0], [0b0110, 0], [2, 1])
    assert cols["pose_dim"] == [0, 5, 6] and cols["pose_off"] == [0, 0, 5]
    assert cols["pose_slots"] == [[], [0, 1, 2, 3, 5], [0, 1, 2, 3, 4, 5]]
    assert cols["intr_off"] == [11, 13] and cols["intr_slots"] == [[0, 3], [0, 1, 2, 3]] and cols["n_c"] == 17


def _stub(n_c=8):
    from pixsfm_amd.api.covariance import BACovariance
    rng = np.random.default_rng(0)
    def spd(n):
        m = rng.normal(size=(n, n))
        return m @ m.T
    pose = np.stack([np.zeros((6, 6)), spd(6)])
    intr = np.zeros((1, 12, 12))
    intr[0][np.ix_([0, 3], [0, 3])] = spd(2)
    points = np.stack([spd(3), np.zeros((3, 3)), np.full((3, 3), np.nan)])
    dense = spd(n_c)
    cov = {"pose": pose, "intrinsics": intr, "points": points, "cameras": dense,
           "columns": {"pose_slots": [[], [0, 1, 2, 3, 4, 5]], "intr_slots": [[0, 3]], "pose_off": [0, 0], "pose_dim": [0, 6],
                       "intr_off": [6], "intr_dim": [2], "n_c": n_c},
           "summary": {"info": 0, "num_camera_unknowns": n_c, "num_singular_points": 1}}
    return cov, BACovariance([10, 20], [7], [100, 200, 300], [2], cov, factor=1.0)


def test_blocks_are_indexed_by_colmap_id():
    cov, c = _stub()
    assert not c.pose_cov(10).any()
    assert np.array_equal(c.point_cov(100), cov["points"][0]) and not c.point_cov(200).any() and np.isnan(c.point_cov(300)).all()
    assert c.intrinsics_cov(7).shape == (4, 4) and np.array_equal(c.intrinsics_cov(7), cov["intrinsics"][0][:4, :4])
    for bad in (lambda: c.pose_cov(11), lambda: c.point_cov(1), lambda: c.intrinsics_cov(8)):
        with pytest.raises(KeyError):
            bad()
    dense, names = c.cameras_cov()
    assert names[:6] == [("pose", 20, k) for k in range(6)] and names[6:] == [("intrinsics", 7, 0), ("intrinsics", 7, 3)]
    assert dense.shape == (8, 8)


def test_half_angle_to_radians_on_a_hand_made_block():
    from pixsfm_amd.api.covariance import half_angle_to_radians
    block = np.arange(36, dtype=np.float64).reshape(6, 6)
    out = half_angle_to_radians(block)
    assert np.array_equal(out[:3, :3], 4.0 * block[:3, :3])            # rotation: angle = 2 x half angle, variance x 4
    assert np.array_equal(out[:3, 3:], 2.0 * block[:3, 3:]) and np.array_equal(out[3:, :3], 2.0 * block[3:, :3])
    assert np.array_equal(out[3:, 3:], block[3:, 3:])
    cov, c = _stub()
    assert np.array_equal(c.pose_cov(20), half_angle_to_radians(cov["pose"][1]))
    dense, _ = c.cameras_cov()
    assert np.array_equal(dense[:3, :3], 4.0 * cov["cameras"][:3, :3]) and np.array_equal(dense[6:, :3], 2.0 * cov["cameras"][6:, :3])


def test_posterior_scale_arithmetic():
    from pixsfm_amd.api.covariance import BACovariance, posterior_factor
    assert posterior_factor(cost=30.0, num_residuals=320, num_parameters=20) == 2.0 * 30.0 / 300
    with pytest.raises(ValueError):
        posterior_factor(1.0, 10, 10)
    cov, _ = _stub()
    c = BACovariance([10, 20], [7], [100, 200, 300], [2], cov, factor=0.2)
    assert np.array_equal(c.point_cov(100), cov["points"][0] * 0.2)
    assert c.summary["factor"] == 0.2


def test_rank_deficiency_text_names_the_gauge():
    from pixsfm_amd.api.covariance import rank_deficiency_message
    columns = {"pose_off": [0, 6], "pose_dim": [6, 6], "intr_off": [12], "intr_dim": [2]}
    text = rank_deficiency_message({"info": 9, "num_camera_unknowns": 14}, columns, [10, 20], [7])
    assert "gauge is not fixed" in text and "column 9 of 14" in text and "pose of image 20" in text
    assert "14 camera-side columns were free" in text and "2 of 2 poses" in text
    text = rank_deficiency_message({"info": 14, "num_camera_unknowns": 14}, columns, [10, 20], [7])
    assert "intrinsics of camera 7" in text


def test_names_are_exported():
    from pixsfm_amd import api
    assert api.estimate_ba_covariance is api.covariance.estimate_ba_covariance and api.BACovariance is api.covariance.BACovariance
    with pytest.raises(ValueError):
        api.estimate_ba_covariance({"strategy": "geometric"}, None, scale="sigma")
