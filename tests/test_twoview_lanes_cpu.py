"""The source of the two-view geometry kernels, run lane by lane on the CPU: csrc/pxr_twoview.hip is compiled as host C++ over
the stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through
an exchange buffer) and held to the numpy reference like the GPU test does -- the sample hash, the five-point solver, the keys
and the stop rule across the four wavefronts of a workgroup, Horn's decomposition, the workgroup sums of the refinement, the
compaction and the host-side validation are checked without a GPU.  What only hardware can show (LDS and scratch behaviour,
occupancy, the device's libm) stays with tests/test_twoview_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import twoview_cases as tv
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "twoview_on_host.cpp")


def _run(emu, batch, qvec=None, tvec=None, **options):
    from pixsfm_amd.engine import _padded_cam_params, two_view_options
    lib, ctx = emu
    off = np.ascontiguousarray(batch["pair_offsets"], np.int64)
    xy1, xy2 = np.ascontiguousarray(batch["xy1"], np.float64), np.ascontiguousarray(batch["xy2"], np.float64)
    pc, cm = np.ascontiguousarray(batch["pair_camera"], np.int32), np.ascontiguousarray(batch["cam_model"], np.int32)
    cp = _padded_cam_params(batch["cam_params"], len(cm))
    T, N = len(off) - 1, len(xy1)
    pq = None if batch.get("prior_qvec") is None else np.ascontiguousarray(batch["prior_qvec"], np.float64)
    pt = None if batch.get("prior_tvec") is None else np.ascontiguousarray(batch["prior_tvec"], np.float64)
    opts = two_view_options(**options)
    q = np.full((T, 4), np.nan) if qvec is None else np.array(qvec, dtype=np.float64)
    t = np.full((T, 3), np.nan) if tvec is None else np.array(tvec, dtype=np.float64)
    E = np.full((T, 9), np.nan)
    st, ni, nt = np.full(T, -9, np.int32), np.full(T, -9, np.int32), np.full(T, -9, np.int32)
    inl, err = np.full(N, 9, np.uint8), np.full(N, -1.0)
    rc = lib.pxr_two_view_geometry(ctx, C.c_int32(T), _p(off), C.c_int64(N), _p(xy1), _p(xy2), _p(pc), C.c_int32(len(cm)), _p(cm), _p(cp),
                                   _p(pq), _p(pt), C.byref(opts), _p(q), _p(t), _p(E), _p(st), _p(ni), _p(nt), _p(inl), _p(err))
    lanes.check(lib, rc)
    return dict(qvec=q, tvec=t, E=E, status=st, n_inliers=ni, n_trials=nt, inlier=inl, err=err)


def test_kernel_source_matches_the_reference_on_the_boundary_batch(emu):
    """Measured (clang -O1, contraction off): max rotation difference 9.7e-16 rad, max translation-direction difference
    1.2e-15 rad, max error difference 3.4e-13 px (before the hypotheses were polished: 1.1e-15, 8.2e-16, 3.4e-13);
    tv.POSE_TOL / tv.ERR_TOL stay at 1000 x the earlier figures (1.1e-12 rad, 3.5e-10 px), below section 19's 1e-7 rad / 1e-6 px."""
    batch, ref = tv.boundary_batch()
    assert {0, 1, 3}.issubset(set(ref["status"]))
    assert np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"] & np.repeat(ref["status"] == 0, np.diff(batch["pair_offsets"])))
    tv.compare(_run(emu, batch), ref, report="lanes vs reference: ")


def test_pose_prior_mode(emu):
    batch, _ = tv.boundary_batch()
    counts = np.diff(batch["pair_offsets"])
    keep = [int(np.flatnonzero(counts == n)[0]) for n in (4, 16, 65, tv.LDS_MATCHES + 1)]
    parts = [tv.single(batch, p) for p in keep]
    sub = dict(batch, pair_offsets=np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int64),
               xy1=np.concatenate([b["xy1"] for b in parts]), xy2=np.concatenate([b["xy2"] for b in parts]),
               pair_camera=batch["pair_camera"][keep], prior_qvec=batch["gt_qvec"][keep], prior_tvec=3.0 * batch["gt_tvec"][keep])
    ref = tv.reference(sub)
    got = _run(emu, sub)
    assert got["status"].tolist() == [1, 0, 0, 0] and (got["n_trials"] == 0).all()
    assert np.array_equal(got["qvec"][1:], sub["prior_qvec"][1:]) and np.array_equal(got["tvec"][1:], sub["prior_tvec"][1:])
    assert np.array_equal(got["inlier"], ref["inlier"]) and np.array_equal(got["n_inliers"], ref["n_inliers"])
    inl = np.concatenate([b["true_inlier"][batch["pair_offsets"][p]:batch["pair_offsets"][p + 1]] for b, p in zip(parts, keep)])
    assert np.array_equal(got["inlier"][4:].astype(bool), inl[4:])


def test_status_codes_and_validation(emu):
    batch = tv.make_pairs([4, 40, 40], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    batch["xy1"][off[1]:off[2]], batch["xy2"][off[1]:off[2]] = batch["xy1"][off[1]], batch["xy2"][off[1]]        # 40 copies of one match
    sq, stv = np.arange(12.0).reshape(3, 4) - 50, np.arange(9.0).reshape(3, 3) - 70
    got = _run(emu, batch, qvec=sq, tvec=stv, min_num_inliers=41)
    assert got["status"].tolist() == [1, 2, 3] and got["n_inliers"].tolist() == [0, 0, 0]
    assert np.array_equal(got["qvec"], sq) and np.array_equal(got["tvec"], stv) and np.isnan(got["E"]).all()
    assert not got["inlier"].any() and np.isnan(got["err"]).all()
    assert got["n_trials"].tolist()[:2] == [0, 10048]
    for change, word in ((dict(pair_offsets=np.array([0, 30, 15, 84], np.int64)), "monotone"),
                         (dict(pair_offsets=np.array([0, 4, 44, 83], np.int64)), "n_matches"),
                         (dict(pair_camera=np.array([[0, 0], [0, 1], [0, 0]], np.int32)), "camera"),
                         (dict(prior_qvec=np.ones((3, 4))), "prior")):
        with pytest.raises(ValueError, match=word):
            _run(emu, dict(batch, **change))


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    host program: pairs down to 5 matches, empty pairs, S + 1 matches; with and without a pose prior."""
    counts = [0, 5, 6, 0, 17, 70, tv.LDS_MATCHES + 1, 0]
    stdout = lanes.sanitized(tmp_path, "twoview_on_host.cpp", "TWOVIEW_ON_HOST_MAIN", *counts)
    lines = [ln for ln in stdout.split("\n") if ln.startswith("pair")]
    assert len(lines) == 2 * len(counts)
    assert "pair 0: 0 matches, status 1, 0 inliers, 0 trials" in lines and any(ln.startswith("pair 6: 1025 matches, status 0") for ln in lines)
