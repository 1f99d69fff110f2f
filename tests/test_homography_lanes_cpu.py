"""The source of the homography kernels, run lane by lane on the CPU: csrc/pxr_homography.hip is compiled as host C++ over the
stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through an
exchange buffer) and held to the numpy reference like the GPU test does -- the sample hash, the four-point solver, the keys and
the floored stop rule across the four wavefronts of a workgroup, the workgroup sums of both refinements, the rotation-only model,
the compaction and the host-side validation are checked without a GPU.  What only hardware can show (LDS and scratch behaviour,
occupancy, the device's libm) stays with tests/test_homography_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import homography_cases as hc
import lanes
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "homography_on_host.cpp")


def _run(emu, batch, H=None, rot_qvec=None, **options):
    from pixsfm_amd.engine import _padded_cam_params, homography_options
    lib, ctx = emu
    off = np.ascontiguousarray(batch["pair_offsets"], np.int64)
    xy1, xy2 = np.ascontiguousarray(batch["xy1"], np.float64), np.ascontiguousarray(batch["xy2"], np.float64)
    pc, cm = np.ascontiguousarray(batch["pair_camera"], np.int32), np.ascontiguousarray(batch["cam_model"], np.int32)
    cp = _padded_cam_params(batch["cam_params"], len(cm))
    T, N = len(off) - 1, len(xy1)
    opts = homography_options(**options)
    Hm = np.full((T, 9), np.nan) if H is None else np.array(H, dtype=np.float64)
    q = np.full((T, 4), np.nan) if rot_qvec is None else np.array(rot_qvec, dtype=np.float64)
    st, ni, nr, nt = (np.full(T, -9, np.int32) for _ in range(4))
    inl, err = np.full(N, 9, np.uint8), np.full(N, -1.0)
    rc = lib.pxr_homography(ctx, C.c_int32(T), _p(off), C.c_int64(N), _p(xy1), _p(xy2), _p(pc), C.c_int32(len(cm)), _p(cm), _p(cp),
                            C.byref(opts), _p(Hm), _p(q), _p(st), _p(ni), _p(nr), _p(nt), _p(inl), _p(err))
    lanes.check(lib, rc)
    return dict(H=Hm, rot_qvec=q, status=st, n_inliers=ni, n_rot_inliers=nr, n_trials=nt, inlier=inl, err=err)


def test_kernel_source_matches_the_reference_on_the_boundary_batch(emu):
    """Measured (clang -O1, contraction off): max difference of H 3.5e-16 (Frobenius, unit-norm H, sign fixed by the inliers), max
    rotation difference 2.3e-16 rad, max error difference 5.7e-13 px; hc.H_TOL / hc.ROT_TOL / hc.ERR_TOL are 1000 x these
    (3.5e-13, 2.3e-13 rad, 5.7e-10 px), below section 19's caps of 1e-7 and 1e-6 px."""
    batch, ref = hc.boundary_batch()
    hc.check_reference(batch, ref)
    hc.compare(_run(emu, batch), ref, report="lanes vs reference: ")


def test_status_codes_and_validation(emu):
    batch = hc.make_pairs(["planar"] * 3, [3, 40, 40], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    batch["xy1"][off[1]:off[2]], batch["xy2"][off[1]:off[2]] = batch["xy1"][off[1]], batch["xy2"][off[1]]        # 40 copies of one match
    sH, sq = np.arange(27.0).reshape(3, 9) - 50, np.arange(12.0).reshape(3, 4) - 70
    got = _run(emu, batch, H=sH, rot_qvec=sq, min_num_inliers=41)
    assert got["status"].tolist() == [1, 2, 3] and got["n_inliers"].tolist() == [0, 0, 0] and got["n_rot_inliers"].tolist() == [0, 0, 0]
    assert np.array_equal(got["H"], sH) and np.array_equal(got["rot_qvec"], sq)
    assert not got["inlier"].any() and np.isnan(got["err"]).all()
    assert got["n_trials"].tolist() == [0, 64, 64]          # need = 41 > n = 40: w is capped at 1, the lower clamp ends both
    for change, word in ((dict(pair_offsets=np.array([0, 30, 15, 83], np.int64)), "monotone"),
                         (dict(pair_offsets=np.array([0, 3, 43, 82], np.int64)), "n_matches"),
                         (dict(pair_camera=np.array([[0, 0], [0, 1], [0, 0]], np.int32)), "camera")):
        with pytest.raises(ValueError, match=word):
            _run(emu, dict(batch, **change))
    with pytest.raises(ValueError, match="option"):
        _run(emu, batch, confidence=1.0)


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    host program: empty pairs, pairs of 4, 5, 17, 70 and S + 1 matches, rotation-only and planar in turn."""
    counts = [0, 4, 5, 0, 70, 70, hc.LDS_MATCHES + 1, 17, 0]
    stdout = lanes.sanitized(tmp_path, "homography_on_host.cpp", "HOMOGRAPHY_ON_HOST_MAIN", *counts)
    lines = [ln for ln in stdout.split("\n") if ln.startswith("pair")]
    assert len(lines) == len(counts)
    assert "pair 0: 0 matches, status 1, 0 inliers, 0 rotation inliers, 0 trials" in lines
    assert any(ln.startswith("pair 6: 1025 matches, status 0") for ln in lines)
    rot, pla = lines[4].split(", "), lines[5].split(", ")    # 70 matches each: an even pair is rotation-only, an odd one planar
    assert rot[1] == pla[1] == "status 0" and rot[2].split()[0] == rot[3].split()[0] and int(pla[3].split()[0]) < int(pla[2].split()[0]) // 2
