"""The source of the absolute-pose kernels, run lane by lane on the CPU: csrc/pxr_abspose.hip is compiled as host C++ over the
stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through an
exchange buffer) and held to the numpy reference like the GPU test does -- the sample hash, the P3P solver, the keys and the
stop rule across the four wavefronts of a workgroup, the workgroup sums of the refinement, the compaction and the host-side
validation are checked without a GPU.  What only hardware can show (LDS behaviour, occupancy, the device's libm) stays with
tests/test_abspose_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import abspose_cases as ac
import lanes
import triangulation_cases as tc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "abspose_on_host.cpp")


def _run(emu, batch, qvec=None, tvec=None, **options):
    from pixsfm_amd.engine import _padded_cam_params, abspose_options
    lib, ctx = emu
    off = np.ascontiguousarray(batch["query_offsets"], np.int64)
    xy, xyz = np.ascontiguousarray(batch["xy"], np.float64), np.ascontiguousarray(batch["xyz"], np.float64)
    qc, cm = np.ascontiguousarray(batch["query_camera"], np.int32), np.ascontiguousarray(batch["cam_model"], np.int32)
    cp = _padded_cam_params(batch["cam_params"], len(cm))
    T, N = len(off) - 1, len(xy)
    opts = abspose_options(**options)
    q = np.full((T, 4), np.nan) if qvec is None else np.array(qvec, dtype=np.float64)
    t = np.full((T, 3), np.nan) if tvec is None else np.array(tvec, dtype=np.float64)
    st, ni, nt = np.full(T, -9, np.int32), np.full(T, -9, np.int32), np.full(T, -9, np.int32)
    inl, err = np.full(N, 9, np.uint8), np.full(N, -1.0)
    rc = lib.pxr_absolute_pose(ctx, C.c_int32(T), _p(off), C.c_int64(N), _p(xy), _p(xyz), _p(qc), C.c_int32(len(cm)), _p(cm), _p(cp),
                               C.byref(opts), _p(q), _p(t), _p(st), _p(ni), _p(nt), _p(inl), _p(err))
    lanes.check(lib, rc)
    return dict(qvec=q, tvec=t, status=st, n_inliers=ni, n_trials=nt, inlier=inl, err=err)


def test_kernel_source_matches_the_reference_on_the_boundary_batch(emu):
    """Measured (clang -O1, contraction off): max rotation difference 9.0e-16 rad, max |dt|/|t|
    2.8e-15, max pixel-error difference 1.7e-12 px."""
    batch, ref = ac.boundary_batch()
    assert {0, 1}.issubset(set(ref["status"]))
    assert np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"] & np.repeat(ref["status"] == 0, np.diff(batch["query_offsets"])))
    ac.compare(_run(emu, batch), ref, report="lanes vs reference: ")


def test_status_codes_and_validation(emu):
    xy, X = ac.collinear_query()
    batch = ac.make_queries([3, len(xy), 40], (1,), seed=5, p_outlier=0.0)
    off = batch["query_offsets"]
    batch["xy"][off[1]:off[2]], batch["xyz"][off[1]:off[2]] = xy, X
    batch["xy"][off[2]:off[3]] = np.random.default_rng(6).uniform(0, 900, (40, 2))        # all outliers
    sq, stv = np.arange(12.0).reshape(3, 4) - 50, np.arange(9.0).reshape(3, 3) - 70
    got = _run(emu, batch, qvec=sq, tvec=stv, min_num_inliers=30)
    assert got["status"].tolist() == [1, 2, 3] and got["n_inliers"].tolist() == [0, 0, 0]
    assert np.array_equal(got["qvec"], sq) and np.array_equal(got["tvec"], stv)
    assert not got["inlier"].any() and np.isnan(got["err"]).all()
    assert got["n_trials"].tolist()[:2] == [0, 4096]
    for change, word in ((dict(query_offsets=np.array([0, 30, 15, 55], np.int64)), "monotone"),
                         (dict(query_offsets=np.array([0, 3, 15, 54], np.int64)), "n_corr"),
                         (dict(query_camera=np.array([0, 1, 0], np.int32)), "camera")):
        with pytest.raises(ValueError, match=word):
            _run(emu, dict(batch, **change))
