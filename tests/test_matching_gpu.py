"""GPU: the matching kernels (csrc/pxr_match.hip) against the reference of tests/matching_cases.py, bit for bit: matches0,
n_matches, and scores0 as uint32 views.  The reference's similarity is the float32 fmaf chain (tests/host/sim_fmaf.c); that the
f32-input MFMA gives those bits is what these tests establish."""
import ctypes as C

import numpy as np
import pytest

import matching_cases as mc

pytestmark = pytest.mark.gpu


def _run(ctx, descs, pairs, **options):
    from pixsfm_amd.engine import MatchProblem
    prob = MatchProblem(ctx, descs, pairs)
    m, s, n = (a.download() for a in prob.run(**options))
    return m, s, n, prob.pair_offsets


def _equal(got, ref, what):
    m, s, n = got[:3]
    rm, rs, rn = ref[:3]
    assert m.dtype == np.int32 and s.dtype == np.float32 and n.dtype == np.int32
    bad = np.flatnonzero(m != rm)
    assert len(bad) == 0, "%s: matches0 differs at %s: got %s, reference %s" % (what, bad[:8], m[bad[:8]], rm[bad[:8]])
    bad = np.flatnonzero(s.view(np.uint32) != rs.view(np.uint32))
    assert len(bad) == 0, "%s: scores0 differs in bits at %s: got %s, reference %s" % (what, bad[:8], s[bad[:8]], rs[bad[:8]])
    assert np.array_equal(n, rn), (what, n, rn)


@pytest.fixture(scope="module")
def shape_cases():
    """descriptors and per-option references of every shape, computed once"""
    out = {}
    for k, shape in enumerate(mc.GPU_SHAPES):
        A, B = mc.pair_case(*shape, seed=100 + k)
        sim = mc.sim_chain(A, B)
        out[shape] = (A, B, {name: mc.match_from_sim(sim, **o) for name, o in mc.OPTION_SETS.items()})
    return out


@pytest.mark.parametrize("shape", mc.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_equal_the_reference_bit_for_bit(ctx, shape_cases, shape):
    A, B, refs = shape_cases[shape]
    kept = 0
    for name, options in mc.OPTION_SETS.items():
        rm, rs, rn = refs[name]
        got = _run(ctx, [A, B], [(0, 1)], **options)
        _equal(got, (rm, rs, np.array([rn], np.int32)), "%s %s" % (shape, name))
        kept += rn
    assert kept > 0


def test_ties_go_to_the_lowest_index(ctx):
    for copies_in_b in (True, False):
        A, B = mc.tie_case(copies_in_b)
        for name in ("NN-mutual", "NN-ratio"):
            rm, rs, rn = mc.match_reference(A, B, mc.CONFS[name])
            got = _run(ctx, [A, B], [(0, 1)], **mc.CONFS[name])
            _equal(got, (rm, rs, np.array([rn], np.int32)), "ties %s %s" % (copies_in_b, name))
        m = _run(ctx, [A, B], [(0, 1)], **mc.CONFS["NN-mutual"])[0]
        if copies_in_b:
            assert m[11] == 5
        else:
            assert m[5] == 11 and m[17] == -1 and m[40] == -1


@pytest.fixture(scope="module")
def batch(ctx):
    descs, pairs = mc.batch_case()
    return descs, pairs, {name: _run(ctx, descs, pairs, **o) for name, o in mc.OPTION_SETS.items()}


def test_batch_equals_the_reference_and_each_pair_alone(ctx, batch):
    descs, pairs, got = batch
    assert [len(d) for d in descs] == [0, 1, 33, 129, 200] and len(pairs) == 6
    for name, options in mc.OPTION_SETS.items():
        m, s, n, off = got[name]
        ref = mc.reference_batch(descs, pairs, options)
        assert np.array_equal(off, ref[3]) and len(m) == off[-1]
        _equal((m, s, n), ref, "batch %s" % name)
    m, s, n, off = got["NN-ratio"]
    for p, (a, b) in enumerate(pairs):
        om, os_, on, _ = _run(ctx, [descs[a], descs[b]], [(0, 1)], **mc.CONFS["NN-ratio"])
        assert om.tobytes() == m[off[p]:off[p + 1]].tobytes() and os_.tobytes() == s[off[p]:off[p + 1]].tobytes() and on[0] == n[p], p
    assert n[3] == 0 and off[4] - off[3] == 0                        # the empty image first: an empty result
    assert (m[off[4]:off[5]] == -1).all() and (s[off[4]:off[5]] == 0).all() and n[4] == 0 and off[5] - off[4] == 33   # second: all -1


def test_swapped_pair_is_consistent_under_the_mutual_check(batch):
    _, pairs, got = batch
    m, _, n, off = got["NN-mutual"]
    assert pairs[1].tolist() == [3, 4] and pairs[2].tolist() == [4, 3]
    ab, ba = m[off[1]:off[2]], m[off[2]:off[3]]
    fwd = {(i, int(j)) for i, j in enumerate(ab) if j >= 0}
    bwd = {(int(i), j) for j, i in enumerate(ba) if i >= 0}
    assert fwd == bwd and len(fwd) == n[1] == n[2] and len(fwd) >= 80
    same = m[off[0]:off[1]]                                          # (4, 4): every descriptor's nearest neighbour is itself
    assert np.array_equal(same, np.arange(200))


def test_two_runs_give_identical_bytes(ctx, batch):
    descs, pairs, got = batch
    for name in ("NN-ratio", "NN-mutual"):
        again = _run(ctx, descs, pairs, **mc.OPTION_SETS[name])
        for x, y in zip(again[:3], got[name][:3]):
            assert x.tobytes() == y.tobytes()


def test_timed_run_reports_three_kernels(ctx, batch):
    from pixsfm_amd.engine import MatchProblem
    descs, pairs, got = batch
    prob = MatchProblem(ctx, descs, pairs)
    out = prob.run(timed=True, **mc.CONFS["NN-ratio"])
    assert set(prob.kernel_ms) == {"tiles", "columns", "mutual"} and all(v >= 0 for v in prob.kernel_ms.values())
    assert out[0].download().tobytes() == got["NN-ratio"][0].tobytes()


INVALID = {
    "offsets not starting at 0": (dict(offsets=[1, 40, 90]), "d_image_offsets"),
    "offsets not monotone": (dict(offsets=[0, 95, 90]), "d_image_offsets"),
    "offsets not ending at n_total": (dict(offsets=[0, 40, 80]), "n_total"),
    "pair index out of range": (dict(pairs=[(0, 1), (1, 2)]), "d_pairs"),
    "negative pair index": (dict(pairs=[(-1, 1)]), "d_pairs"),
    "D = 0": (dict(dim=0), "dim"),
    "D = 513": (dict(dim=513), "dim"),
}


@pytest.mark.parametrize("case", list(INVALID))
def test_invalid_input_is_refused_and_nothing_is_written(ctx, case):
    from pixsfm_amd.engine import match_options
    change, word = INVALID[case]
    rng = np.random.default_rng(8)
    desc = mc.unit_rows(rng, 90, 16)
    offsets = np.array(change.get("offsets", [0, 40, 90]), dtype=np.int64)
    pairs = np.array(change.get("pairs", [(0, 1), (1, 0)]), dtype=np.int32)
    dim = change.get("dim", 16)
    pair_off = np.array([0, 40, 90][:len(pairs) + 1], dtype=np.int64)
    d_desc, d_off, d_pairs, d_poff = (ctx.to_device(x) for x in (desc, offsets, pairs, pair_off))
    sm, ss, sn = np.full(90, 77, np.int32), np.full(90, 0.25, np.float32), np.full(len(pairs), 55, np.int32)
    d_m, d_s, d_n = ctx.to_device(sm), ctx.to_device(ss), ctx.to_device(sn)
    opts = match_options()
    rc = ctx.lib.pxr_match_descriptors(ctx.handle, 2, d_off.ptr, 90, dim, d_desc.ptr, len(pairs), d_pairs.ptr, d_poff.ptr, C.byref(opts),
                                       d_m.ptr, d_s.ptr, d_n.ptr)
    msg = ctx.lib.pxr_last_error().decode()
    assert rc == -1                                                  # PXR_EINVAL
    assert "pxr_match_descriptors" in msg and word in msg, msg
    assert np.array_equal(d_m.download(), sm) and np.array_equal(d_s.download(), ss) and np.array_equal(d_n.download(), sn)


def test_no_pairs_and_only_empty_images_return_without_work(ctx):
    m, s, n, off = _run(ctx, [np.empty((0, 8), np.float32), mc.unit_rows(np.random.default_rng(1), 5, 8)], np.empty((0, 2), np.int32))
    assert len(m) == 0 and len(s) == 0 and len(n) == 0
    m, s, n, off = _run(ctx, [np.empty((0, 8), np.float32), np.empty((0, 8), np.float32)], [(0, 1), (1, 1)])
    assert len(m) == 0 and len(s) == 0 and n.tolist() == [0, 0]


def test_api_equals_the_cpu_seam_and_splits_into_launches(ctx):
    from pixsfm_amd.api import DescriptorMatcher
    desc, owner, pairs = mc.scene()
    want_m, want_s = [], []
    for a, b in pairs:
        m, s, _ = mc.match_reference(desc[a], desc[b], mc.CONFS["NN-ratio"])
        idx = np.flatnonzero(m >= 0)
        want_m.append(np.stack([idx, m[idx]], -1).astype(np.uint64))
        want_s.append(s[idx])
    matcher = DescriptorMatcher.create("NN-ratio", ctx=ctx)
    got_m, got_s = matcher.match_pairs(desc, pairs)
    assert matcher.num_launches == 1
    rows = [len(desc[a]) for a, _ in pairs]
    assert rows == [58, 58, 58, 58, 59, 59, 59, 55, 55, 48]
    bound = 232                                                      # 4 x 58 | 3 x 59 + 55 | 55 + 48: three launches
    split = DescriptorMatcher.create({"ratio_threshold": 0.8, "max_batch_rows": bound}, ctx=ctx)
    split_m, split_s = split.match_pairs(desc, pairs)
    assert split.num_launches == 3, (split.num_launches, rows, bound)
    for lists in ((got_m, got_s), (split_m, split_s)):
        assert len(lists[0]) == len(pairs)
        for p in range(len(pairs)):
            assert lists[0][p].dtype == np.uint64 and np.array_equal(lists[0][p], want_m[p]), p
            assert lists[1][p].dtype == np.float32 and lists[1][p].tobytes() == want_s[p].tobytes(), p
