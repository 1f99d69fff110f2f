"""The source of the fundamental-matrix kernels, run lane by lane on the CPU: csrc/pxr_fundamental.hip is compiled as host C++ over
the stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through an
exchange buffer) and held to the numpy reference like the GPU test does -- the sample hash at seven indices, the seven-point
solver with its cubic and Sturm chain, the keys and the stop rule across the four wavefronts of a workgroup, the workgroup sums of
the rank-2 refinement, the compaction and the host-side validation are checked without a GPU.  What only hardware can show (LDS
and scratch behaviour, occupancy, the device's libm) stays with tests/test_fundamental_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import fundamental_cases as fc
import lanes
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "fundamental_on_host.cpp")


def _run(emu, batch, F=None, **options):
    from pixsfm_amd.engine import _padded_cam_params, fundamental_options
    lib, ctx = emu
    off = np.ascontiguousarray(batch["pair_offsets"], np.int64)
    xy1, xy2 = np.ascontiguousarray(batch["xy1"], np.float64), np.ascontiguousarray(batch["xy2"], np.float64)
    pc, cm = np.ascontiguousarray(batch["pair_camera"], np.int32), np.ascontiguousarray(batch["cam_model"], np.int32)
    cp = _padded_cam_params(batch["cam_params"], len(cm))
    T, N = len(off) - 1, len(xy1)
    opts = fundamental_options(**options)
    Fm = np.full((T, 9), np.nan) if F is None else np.array(F, dtype=np.float64)
    st, ni, nt = (np.full(T, -9, np.int32) for _ in range(3))
    inl, err = np.full(N, 9, np.uint8), np.full(N, -1.0)
    rc = lib.pxr_fundamental(ctx, C.c_int32(T), _p(off), C.c_int64(N), _p(xy1), _p(xy2), _p(pc), C.c_int32(len(cm)), _p(cm), _p(cp),
                             C.byref(opts), _p(Fm), _p(st), _p(ni), _p(nt), _p(inl), _p(err))
    lanes.check(lib, rc)
    return dict(F=Fm, status=st, n_inliers=ni, n_trials=nt, inlier=inl, err=err)


def test_kernel_source_matches_the_reference_on_the_boundary_batch(emu):
    """Measured (clang -O1, contraction off): max difference of F 2.9e-15 (Frobenius, unit-norm F, sign fixed by the largest
    entry), max error difference 4.6e-13 px; fc.F_TOL / fc.ERR_TOL are 1000 x these (2.9e-12, 4.6e-10 px), below section 19's
    caps of 1e-7 and 1e-6 px."""
    batch, ref = fc.boundary_batch()
    fc.check_reference(batch, ref)
    fc.compare(_run(emu, batch), ref, report="lanes vs reference: ")


def test_status_codes_and_validation(emu):
    batch = fc.make_pairs(["general"] * 3, [6, 40, 40], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    sF = np.arange(27.0).reshape(3, 9) - 50
    # seven copies of one match: every sample is the same rank-1 system, no hypothesis, and the stop rule runs to max_num_trials
    one = dict(fc.single(batch, 1), pair_offsets=np.array([0, 7], np.int64), xy1=np.repeat(batch["xy1"][off[1]:off[1] + 1], 7, 0),
               xy2=np.repeat(batch["xy2"][off[1]:off[1] + 1], 7, 0))
    got = _run(emu, one, F=sF[:1])
    assert got["status"].tolist() == [2] and got["n_inliers"].tolist() == [0] and got["n_trials"].tolist() == [10048]
    assert np.array_equal(got["F"], sF[:1]) and not got["inlier"].any() and np.isnan(got["err"]).all()
    got = _run(emu, batch, F=sF, min_num_inliers=41)
    assert got["status"].tolist() == [1, 3, 3] and got["n_inliers"].tolist() == [0, 0, 0]
    assert np.array_equal(got["F"], sF)
    assert not got["inlier"].any() and np.isnan(got["err"]).all()
    assert got["n_trials"].tolist() == [0, 64, 64]
    for change, word in ((dict(pair_offsets=np.array([0, 30, 15, 86], np.int64)), "monotone"),
                         (dict(pair_offsets=np.array([0, 6, 46, 85], np.int64)), "n_matches"),
                         (dict(pair_camera=np.array([[0, 1], [2, 6], [4, 5]], np.int32)), "camera")):
        with pytest.raises(ValueError, match=word):
            _run(emu, dict(batch, **change))
    with pytest.raises(ValueError, match="option"):
        _run(emu, batch, confidence=1.0)


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    host program: empty pairs, pairs of 7, 8, 17, 70 and S + 1 matches, the odd ones through a focal length x 0.7."""
    counts = [0, 7, 8, 0, 70, 70, fc.LDS_MATCHES + 1, 17, 0]
    stdout = lanes.sanitized(tmp_path, "fundamental_on_host.cpp", "FUNDAMENTAL_ON_HOST_MAIN", *counts)
    lines = [ln for ln in stdout.split("\n") if ln.startswith("pair")]
    assert len(lines) == len(counts)
    assert "pair 0: 0 matches, status 1, 0 inliers, 0 trials" in lines
    assert any(ln.startswith("pair 6: 1025 matches, status 0") for ln in lines)
    true_f, wrong_f = lines[4].split(", "), lines[5].split(", ")     # 70 matches each, 17 of them outliers: the focal length does not matter
    assert true_f[1] == wrong_f[1] == "status 0" and int(true_f[2].split()[0]) >= 50 and int(wrong_f[2].split()[0]) >= 50
