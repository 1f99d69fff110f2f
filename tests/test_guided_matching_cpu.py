"""Guided matching without a GPU: the symbols, the reference of tests/guided_matching_cases.py against itself (thr = inf is the
unguided reference; the vectorised statement equals the per-row loops), the model and threshold the Python layer picks, argument
errors, and the repeated-structure scene on the reference alone."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import guided_matching_cases as gc
import matching_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, np.flatnonzero(got[0] != ref[0])[:8])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), what
    assert got[2] == ref[2], what


def test_symbols_are_declared_and_exported():
    from pixsfm_amd import _lib, api
    header = open(os.path.join(ROOT, "include", "pixsfm_hip.h")).read()
    for name in ("pxr_match_guided", "pxr_match_guided_timed"):
        assert re.search(r"\bint %s\(" % name, header)
        assert name in _lib.declared_symbols()
    assert (_lib.GUIDE_EPIPOLAR, _lib.GUIDE_HOMOGRAPHY) == (gc.EPIPOLAR, gc.HOMOGRAPHY) == (0, 1)
    assert re.search(r"#define PXR_GUIDE_EPIPOLAR\s+0\b", header) and re.search(r"#define PXR_GUIDE_HOMOGRAPHY\s+1\b", header)
    assert callable(api.DescriptorMatcher.match_pairs_guided) and callable(api.DescriptorMatcher.match_raw_guided)
    assert callable(api.guided_model) and callable(api.guided_threshold)
    from pixsfm_amd.engine import MatchProblem
    assert callable(MatchProblem.run_guided)


def test_an_infinite_threshold_is_the_unguided_reference():
    c = gc.gated_pair(129, 65, 128, gc.EPIPOLAR, seed=3)
    assert gc.admissible(c["kind"], c["M"], np.inf, c["xy_a"], c["xy_b"]).all()
    for name, options in mc.OPTION_SETS.items():
        got = gc.guided_reference(c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], np.inf, **options)
        _equal(got, mc.match_reference(c["A"], c["B"], options), name)


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
def test_two_statements_of_the_reference_agree(kind):
    cases = {"70x90x5": gc.gated_pair(70, 90, 5, gc.KINDS[kind], seed=5), "edge": gc.edge_pair(gc.KINDS[kind])}
    for what, c in cases.items():
        frac = gc.admissible(c["kind"], c["M"], c["thr"], c["xy_a"], c["xy_b"]).mean()
        assert 0.02 < frac < 0.3, frac
        for name, options in mc.OPTION_SETS.items():
            args = (c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], c["thr"])
            _equal(gc.guided_reference_loops(*args, **options), gc.guided_reference(*args, **options), "%s %s" % (what, name))


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
def test_generators_do_what_they_say(kind):
    k = gc.KINDS[kind]
    gc.check_edge_pair(gc.edge_pair(k), lambda c, **o: gc.guided_reference(c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], c["thr"], **o))
    c = gc.gated_pair(129, 65, 128, k, seed=9)
    frac = gc.admissible(c["kind"], c["M"], c["thr"], c["xy_a"], c["xy_b"]).mean()
    assert 0.1 <= frac <= 0.3, frac
    kept = gc.guided_reference(c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], c["thr"], **mc.CONFS["NN-ratio"])[2]
    assert kept >= 30, kept                                  # 39 descriptors are shared: the matches survive the gate
    descs, xy, pairs, kinds, models, thrs = gc.gated_batch()
    ref = gc.reference_batch(descs, xy, pairs, kinds, models, thrs, mc.CONFS["NN-mutual"])
    assert ref[2][-1] == 0 and ref[2][1] > 0 and ref[2][2] > 0 and not np.array_equal(ref[0][200:329], ref[0][329:458])


def test_guided_model_on_every_class():
    from pixsfm_amd.api import guided_model
    from pixsfm_amd.api.fundamental import DECIDING_MODEL
    from pixsfm_amd.api.homography import CONFIGS
    E, F, H = np.eye(3), 2 * np.eye(3), 3 * np.eye(3)
    for config in CONFIGS:
        letter = DECIDING_MODEL[config]
        got = guided_model({"success": True, "config": config, "E": E, "F": F, "H": H})
        if letter is None:
            assert config == "DEGENERATE" and got is None
        else:
            assert got[0] == letter and np.array_equal(got[1], {"E": E, "F": F, "H": H}[letter]) and got[1].dtype == np.float64
        assert guided_model({"success": True, "config": config, "E": None, "F": None, "H": None}) is None
    assert {DECIDING_MODEL[c] for c in CONFIGS} == {"E", "F", "H", None}
    assert guided_model({"success": False}) is None
    assert guided_model({"success": False, "config": "CALIBRATED"}) is None          # no "E": the estimator failed
    got = guided_model({"success": True, "E": E.tolist()})
    assert got[0] == "E" and np.array_equal(got[1], E)
    with pytest.raises(ValueError, match="unknown configuration"):
        guided_model({"success": True, "config": "WATERMARK", "E": E})


def test_thresholds_are_the_estimators_own():
    from pixsfm_amd.api import guided_threshold
    cam_a = NS(model_id=0, params=np.array([800.0, 320.0, 240.0]))                   # SIMPLE_PINHOLE: f
    cam_b = NS(model_id=1, params=np.array([1000.0, 1500.0, 320.0, 240.0]))          # PINHOLE: (fx + fy) / 2 = 1250
    assert guided_threshold("E", cam_a, cam_b, 4.0) == (4.0 / 800.0 + 4.0 / 1250.0) / 2 == 0.0041
    assert guided_threshold("F", cam_a, cam_b, 4.0) == 0.0041
    assert guided_threshold("H", cam_a, cam_b, 4.0) == 4.0 / 1250.0 == 0.0032
    assert guided_threshold("H", cam_b, cam_a, 2.0) == 2.0 / 800.0 == 0.0025
    with pytest.raises(ValueError, match="unknown model"):
        guided_threshold("R", cam_a, cam_b, 4.0)


def test_argument_errors():
    from pixsfm_amd.api import DescriptorMatcher
    matcher = DescriptorMatcher.create("NN-ratio")
    d = {"a": np.zeros((3, 8), np.float32), "b": np.zeros((4, 8), np.float32)}
    kp = {"a": np.zeros((3, 2)), "b": np.zeros((4, 2))}
    cams = {n: NS(model_id=0, params=np.array([100.0, 0.0, 0.0])) for n in d}
    geom = [{"success": True, "E": np.eye(3)}]
    with pytest.raises(ValueError, match="same length"):
        matcher.match_pairs_guided(d, kp, cams, [("a", "b")], [])
    with pytest.raises(ValueError, match="max_error"):
        matcher.match_pairs_guided(d, kp, cams, [("a", "b")], geom, max_error=-1.0)
    with pytest.raises(ValueError, match="max_error"):
        matcher.match_pairs_guided(d, kp, cams, [("a", "b")], geom, max_error=float("nan"))
    with pytest.raises(KeyError, match="no keypoints or camera"):
        matcher.match_pairs_guided(d, {"a": kp["a"]}, cams, [("a", "b")], geom)
    with pytest.raises(KeyError, match="no descriptors"):
        matcher.match_pairs_guided(d, kp, cams, [("a", "c")], geom)
    with pytest.raises(TypeError):
        matcher.match_pairs_guided(d, kp, cams, [("a", "b")], geom, max_err=1.0)
    for wrong in (np.zeros((6, 2)), np.zeros((2, 2)), np.zeros((3, 1)), np.zeros(6)):       # not one row of >= 2 per descriptor
        with pytest.raises(ValueError, match="keypoints of 'a' must be"):
            matcher.match_pairs_guided(d, dict(kp, a=wrong), cams, [("a", "b")], geom)
    # an image that only pairs without a model name needs no keypoints or camera, and may be empty
    d["e"] = np.zeros((0, 8), np.float32)
    m, s = matcher.match_pairs_guided(d, kp, cams, [("e", "a"), ("a", "e")], [{"success": False}, {"success": False}])
    assert [x.shape for x in m] == [(0, 2), (0, 2)]
    raw = matcher.match_raw_guided(d, kp, cams, [("e", "a"), ("a", "e")], [{"success": False}, {"success": False}])
    assert len(raw[0]["matches0"]) == 0 and raw[1]["matches0"].tolist() == [-1, -1, -1]
    # pairs without a usable model touch no GPU and come back empty
    m, s = matcher.match_pairs_guided(d, kp, cams, [("a", "b"), ("b", "a")], [{"success": False}, {"success": True, "config": "DEGENERATE"}])
    assert [x.shape for x in m] == [(0, 2), (0, 2)] and [x.shape for x in s] == [(0,), (0,)] and m[0].dtype == np.uint64
    raw = matcher.match_raw_guided(d, kp, cams, [("a", "b")], [{"success": False}])
    assert raw[0]["matches0"].tolist() == [-1, -1, -1] and raw[0]["matching_scores0"].tolist() == [0, 0, 0]


def test_repeated_structure_on_the_reference():
    """Conditions, not measurements: what guided matching is for."""
    s = gc.twin_scene()
    n1, n2 = s["pair"]
    uv, (A, B) = gc.twin_normalised(s), (s["descriptors"][n1], s["descriptors"][n2])
    thr = (4.0 / s["focal"] + 4.0 / s["focal"]) / 2
    adm = gc.admissible(gc.EPIPOLAR, s["E"], thr, uv[n1], uv[n2])
    assert adm[np.arange(len(A)), s["partner"]].all()                                # the true partner is always a candidate
    unguided = mc.match_reference(A, B, mc.CONFS["NN-ratio"])
    guided = gc.guided_reference(A, B, uv[n1], uv[n2], gc.EPIPOLAR, s["E"], thr, **mc.CONFS["NN-ratio"])
    print("admissible per row %.1f, unguided NN-ratio %d, guided right / wrong %s" % (adm.sum(1).mean(), unguided[2],
                                                                                   gc.right_wrong(guided[0], s["partner"])))
    assert unguided[2] <= 20
    right, wrong = gc.right_wrong(guided[0], s["partner"])
    assert right >= 360 and wrong == 0
