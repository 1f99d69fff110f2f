"""GPU: the guided matching kernels (pxr_match_guided, csrc/pxr_match.hip) through the C-ABI against the reference of
tests/guided_matching_cases.py, bit for bit: matches0, n_matches, and scores0 as uint32 views.  No tolerance anywhere: every
compared quantity is an integer or a float32 that the specification fixes."""
import ctypes as C

import numpy as np
import pytest

import guided_matching_cases as gc
import matching_cases as mc
from test_guided_matching_lanes_cpu import SENTINEL, SHAPES, guided_call, invalid_calls, valid_call
from test_matching_gpu import _equal

pytestmark = pytest.mark.gpu
GPU_SHAPES = SHAPES + [(40, 40, 512)]        # with (70, 90, 130): all three instantiations of the tile kernel


def _run(ctx, *args, **kw):
    """pxr_match_guided over device copies of the arrays; the outputs start from SENTINEL.  PXR_EINVAL: ValueError, after
    checking that no output byte changed."""
    def call(n_images, off, n_total, dim, desc, kp, n_pairs, pairs, poff, kinds, models, thrs, opts, m, s, n):
        dev = [None if a is None else ctx.to_device(a) for a in (off, desc, kp, pairs, poff, kinds, models, thrs, m, s, n)]
        d_off, d_desc, d_kp, d_pairs, d_poff, d_kinds, d_models, d_thrs, d_m, d_s, d_n = dev
        ptr = lambda d: None if d is None else d.ptr          # noqa: E731
        rc = ctx.lib.pxr_match_guided(ctx.handle, n_images, d_off.ptr, n_total, dim, d_desc.ptr, ptr(d_kp), n_pairs, d_pairs.ptr, d_poff.ptr,
                                      ptr(d_kinds), ptr(d_models), ptr(d_thrs), C.byref(opts), d_m.ptr, d_s.ptr, d_n.ptr)
        m[...], s[...], n[...] = d_m.download(), d_s.download(), d_n.download()
        return rc
    rc, m, s, n = guided_call(call, *args, **kw)
    if rc:
        assert rc == -1 and (m == SENTINEL).all() and (s == SENTINEL).all() and (n == SENTINEL).all(), "an error wrote to the outputs"
        raise ValueError(ctx.lib.pxr_last_error().decode())
    return m, s, n


def _run_case(ctx, c, thr=None, **options):
    return _run(ctx, [c["A"], c["B"]], [c["xy_a"], c["xy_b"]], [(0, 1)], [c["kind"]], [c["M"]], [c["thr"] if thr is None else thr], **options)


def _reference(c, **options):
    rm, rs, rn = gc.guided_reference(c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], c["thr"], **options)
    return rm, rs, np.array([rn], np.int32)


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_equal_the_reference_bit_for_bit(ctx, shape, kind):
    c = gc.gated_pair(*shape, gc.KINDS[kind], seed=200 + GPU_SHAPES.index(shape))
    kept = 0
    for name, options in mc.OPTION_SETS.items():
        ref = _reference(c, **options)
        _equal(_run_case(ctx, c, **options), ref, "%s %s %s" % (shape, kind, name))
        kept += ref[2][0]
    assert kept > 0 or shape[0] == 1 or shape[1] == 1


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
def test_planted_rows_and_columns(ctx, kind):
    c = gc.edge_pair(gc.KINDS[kind])
    gc.check_edge_pair(c, lambda case, **o: _run_case(ctx, case, **o))
    for name, options in mc.OPTION_SETS.items():
        _equal(_run_case(ctx, c, **options), _reference(c, **options), "edge %s %s" % (kind, name))


def test_an_infinite_threshold_is_the_unguided_matcher_byte_for_byte(ctx):
    from pixsfm_amd.engine import MatchProblem
    c = gc.gated_pair(129, 65, 128, gc.EPIPOLAR, seed=3)
    for name, options in mc.OPTION_SETS.items():
        m, s, n = _run_case(ctx, c, thr=np.inf, **options)
        um, us, un = (a.download() for a in MatchProblem(ctx, [c["A"], c["B"]], [(0, 1)]).run(**options))
        assert m.tobytes() == um.tobytes() and s.tobytes() == us.tobytes() and n.tobytes() == un.tobytes(), name
        assert n[0] > 0


def test_batch_equals_the_reference_each_pair_alone_and_itself(ctx):
    descs, xy, pairs, kinds, models, thrs = gc.gated_batch()
    for name, options in mc.OPTION_SETS.items():
        ref = gc.reference_batch(descs, xy, pairs, kinds, models, thrs, options)
        got = _run(ctx, descs, xy, pairs, kinds, models, thrs, **options)
        _equal(got, ref, "batch %s" % name)
    m, s, n = got = _run(ctx, descs, xy, pairs, kinds, models, thrs, **mc.CONFS["NN-ratio"])
    again = _run(ctx, descs, xy, pairs, kinds, models, thrs, **mc.CONFS["NN-ratio"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))                    # two runs: identical bytes
    off = gc.reference_batch(descs, xy, pairs, kinds, models, thrs, mc.CONFS["NN-ratio"])[3]
    for p, (a, b) in enumerate(pairs):
        om, os_, on = _run(ctx, [descs[a], descs[b]], [xy[a], xy[b]], [(0, 1)], [kinds[p]], [models[p]], [thrs[p]], **mc.CONFS["NN-ratio"])
        assert om.tobytes() == m[off[p]:off[p + 1]].tobytes() and os_.tobytes() == s[off[p]:off[p + 1]].tobytes() and on[0] == n[p], p
    assert n[7] == 0 and (m[off[7]:off[8]] == -1).all()                                    # the model of all NaN
    assert n[1] > 0 and n[2] > 0 and m[off[1]:off[2]].tobytes() != m[off[2]:off[3]].tobytes()   # one image pair, two models


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    for change, word in invalid_calls():
        kw = valid_call()
        kw.update(change)
        with pytest.raises(ValueError, match="pxr_match_guided.*" + word):
            _run(ctx, **kw)
    m, s, n = _run(ctx, **valid_call())
    assert (m != SENTINEL).all() and (n >= 0).all()


def test_matcher_on_repeated_structure(ctx):
    """DescriptorMatcher.match_pairs_guided on the twin scene, under the E that TwoViewVerifier finds from the NN-mutual matches."""
    from pixsfm_amd.api import DescriptorMatcher, TwoViewVerifier, guided_model, guided_threshold
    from pixsfm_amd.api.reconstruction import Camera
    from pixsfm_amd.engine import image_to_world
    s = gc.twin_scene()
    n1, n2 = pair = s["pair"]
    cams = {n: Camera(k + 1, model, 1000, 1000, params) for k, (n, (model, params)) in enumerate(s["cameras"].items())}
    desc, kps, partner = s["descriptors"], s["keypoints"], s["partner"]
    mutual, _ = DescriptorMatcher.create("NN-mutual", ctx).match_pairs(desc, [pair])
    _, _, geoms = TwoViewVerifier.create(None, ctx).verify_pairs(kps, cams, [pair], mutual)
    assert geoms[0]["success"]
    matcher = DescriptorMatcher.create("NN-ratio", ctx)
    unguided, _ = matcher.match_pairs(desc, [pair])
    (guided, empty), (scores, _) = matcher.match_pairs_guided(desc, kps, cams, [pair, pair], [geoms[0], {"success": False}])
    assert empty.shape == (0, 2) and matcher.num_launches == 2                            # the pair without a model is not launched
    # the reference on the same model, keypoints normalised by the same kernel
    uv = {n: image_to_world(ctx, [cams[n].model_id], [cams[n].params], kps[n])[0] for n in pair}
    letter, E = guided_model(geoms[0])
    rm, rs, rn = gc.guided_reference(desc[n1], desc[n2], uv[n1], uv[n2], gc.EPIPOLAR, E, guided_threshold(letter, cams[n1], cams[n2], 4.0),
                                     **mc.CONFS["NN-ratio"])
    kept = np.flatnonzero(rm >= 0)
    assert letter == "E" and np.array_equal(guided, np.stack([kept, rm[kept]], -1).astype(np.uint64))
    assert np.array_equal(scores.view(np.uint32), rs[kept].view(np.uint32))
    right = int((guided[:, 1] == partner[guided[:, 0].astype(np.int64)]).sum())
    print("unguided NN-ratio %d matches; guided %d right, %d wrong" % (len(unguided[0]), right, len(guided) - right))
    assert len(unguided[0]) <= 20 and right >= 360 and len(guided) - right == 0


def test_empty_images_pairs_without_a_model_and_the_split_by_rows(ctx):
    """An image without features on either side of a live pair, one that only a pair without a model names (it needs no keypoints
    or camera), and conf max_batch_rows splitting the guided launch: the same results as one launch."""
    from pixsfm_amd.api import DescriptorMatcher
    from pixsfm_amd.api.reconstruction import Camera
    s = gc.twin_scene()
    n1, n2 = s["pair"]
    cams = {n: Camera(k + 1, model, 1000, 1000, params) for k, (n, (model, params)) in enumerate(s["cameras"].items())}
    cams["empty.jpg"] = cams[n1]
    desc = dict(s["descriptors"], **{"empty.jpg": np.zeros((0, 64), np.float32), "unseen.jpg": np.zeros((0, 64), np.float32)})
    kps = dict(s["keypoints"], **{"empty.jpg": np.zeros((0, 2))})
    E = {"success": True, "E": s["E"]}
    pairs = [(n1, n2), (n2, n1), (n1, "empty.jpg"), ("empty.jpg", n2), ("unseen.jpg", n1), (n1, n2)]
    geoms = [E, {"success": True, "E": s["E"].T}, E, E, {"success": False}, {"success": True, "config": "DEGENERATE"}]
    one = DescriptorMatcher.create("NN-ratio", ctx)
    m, sc = one.match_pairs_guided(desc, kps, cams, pairs, geoms)
    assert one.num_launches == 1 and [len(x) for x in m[2:]] == [0, 0, 0, 0]
    right = int((m[0][:, 1] == s["partner"][m[0][:, 0].astype(np.int64)]).sum())
    assert right >= 360 and right == len(m[0])
    assert {(int(a), int(b)) for a, b in m[0]} == {(int(b), int(a)) for a, b in m[1]}        # (b, a) under E^t: the same pairs
    split = DescriptorMatcher.create(dict(one.conf, max_batch_rows=500), ctx)
    ms, ss = split.match_pairs_guided(desc, kps, cams, pairs, geoms)
    assert split.num_launches == 3                                                             # 400 | 400 | 400 + 0 rows
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m + sc, ms + ss))
    raw = one.match_raw_guided(desc, kps, cams, pairs, geoms)
    assert (raw[2]["matches0"] == -1).all() and len(raw[2]["matches0"]) == 400 and len(raw[3]["matches0"]) == 0
