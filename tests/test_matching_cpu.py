"""CPU: the descriptor matcher's reference (tests/matching_cases.py) against independent statements of the same rules, the conf
handling of DescriptorMatcher, and the shapes of its outputs all the way into the match graph -- with the kernels replaced by the
reference through DescriptorMatcher._run, so nothing here needs a GPU."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import matching_cases as mc
from pixsfm_amd import _lib
from pixsfm_amd.api import DescriptorMatcher, build_matching_graph, pairs_2d3d_from_matches
from pixsfm_amd.api import base
from pixsfm_amd.engine import MATCH_CONFS, match_options


class ReferenceMatcher(DescriptorMatcher):
    """DescriptorMatcher with the kernels replaced by the numpy reference (the test seam: _run)."""

    def _run(self, descriptors, pair_indices):
        self.num_launches += 1
        return [mc.match_reference(descriptors[a], descriptors[b], mc_options(self.options()))[:2] for a, b in pair_indices]


def mc_options(o):
    return dict(ratio_threshold=float(o["ratio_threshold"] or 0.0), distance_threshold=float(o["distance_threshold"] or 0.0),
                do_mutual_check=bool(o["do_mutual_check"]))


# ---- the similarity ------------------------------------------------------------------------------------------------------------------
def test_sim_chain_is_within_the_float32_chain_bound_of_float64():
    A, B = mc.pair_case(64, 64, 128, seed=1)
    sim = mc.sim_chain(A, B)
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    exact = a64 @ b64.T
    bound = 128 * 2.0 ** -24 * (np.abs(a64) @ np.abs(b64).T)
    assert sim.dtype == np.float32 and (np.abs(sim.astype(np.float64) - exact) <= bound).all()


def test_sim_chain_really_chains():
    """A float64 accumulation rounded once at the end is not the chain: it differs in bits somewhere on 64 x 64 x 128."""
    A, B = mc.pair_case(64, 64, 128, seed=1)
    sim = mc.sim_chain(A, B)
    once = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32)
    assert (sim.view(np.uint32) != once.view(np.uint32)).any()


def test_odd_dimension_and_empty_sides():
    A, B = mc.pair_case(7, 9, 5, seed=2)
    Ap, Bp = np.pad(A, ((0, 0), (0, 11))), np.pad(B, ((0, 0), (0, 11)))          # zero padding of k changes no bit
    assert np.array_equal(mc.sim_chain(A, B).view(np.uint32), mc.sim_chain(Ap, Bp).view(np.uint32))
    m, s, n = mc.match_reference(A, np.empty((0, 5), np.float32))
    assert m.tolist() == [-1] * 7 and s.tolist() == [0.0] * 7 and n == 0
    m, s, n = mc.match_reference(np.empty((0, 5), np.float32), B)
    assert len(m) == 0 and len(s) == 0 and n == 0


# ---- the rules, stated a second time in torch ----------------------------------------------------------------------------------------
def _torch_rules(sim, ratio_threshold, distance_threshold, do_mutual_check):
    sim = torch.from_numpy(sim)
    na, nb = sim.shape

    def nn(s):
        top, idx = s.topk(2, dim=1)
        d = 2 * (1 - top)
        ok = torch.ones(s.shape[0], dtype=torch.bool)
        if ratio_threshold > 0:
            ok &= d[:, 0] <= torch.tensor(ratio_threshold * ratio_threshold, dtype=torch.float64).to(torch.float32) * d[:, 1]
        if distance_threshold > 0:
            ok &= d[:, 0] <= torch.tensor(distance_threshold * distance_threshold, dtype=torch.float64).to(torch.float32)
        return torch.where(ok, idx[:, 0], torch.tensor(-1)), top[:, 0]

    m0, s1 = nn(sim)
    if do_mutual_check:
        m1, _ = nn(sim.t().contiguous())
        back = torch.gather(m1, 0, torch.where(m0 >= 0, m0, torch.tensor(0)))
        m0 = torch.where((m0 >= 0) & (back == torch.arange(na)), m0, torch.tensor(-1))
    scores = torch.where(m0 >= 0, (s1 + 1) / 2, torch.tensor(0.0))
    return m0.numpy().astype(np.int32), scores.numpy()


@pytest.mark.parametrize("name", list(mc.OPTION_SETS))
@pytest.mark.parametrize("shape,seed", [((70, 90, 64), 4), ((129, 65, 128), 5), ((40, 40, 32), 6)])
def test_reference_equals_the_rules_in_torch(name, shape, seed):
    A, B = mc.pair_case(*shape, seed=seed)
    sim = mc.sim_chain(A, B)
    for s in (sim, sim.T):                                      # tie-free: no two equal similarities in a row or a column
        srt = np.sort(s, axis=1)
        assert (np.diff(srt, axis=1) > 0).all()
    opts = mc.OPTION_SETS[name]
    m, sc, n = mc.match_from_sim(sim, **opts)
    tm, tsc = _torch_rules(sim, **opts)
    assert np.array_equal(m, tm) and np.array_equal(sc.view(np.uint32), tsc.view(np.uint32)) and n == (tm >= 0).sum()
    assert 0 < n < shape[0]                                     # the case exercises both outcomes


def test_ties_go_to_the_lowest_index_and_fail_the_ratio_test():
    A, B = mc.tie_case(copies_in_b=True)
    m, s, _ = mc.match_reference(A, B, mc.CONFS["NN-mutual"])
    assert m[11] == 5                                           # forward: lowest of 5, 17, 40; backward: column 5's best is row 11
    m, _, _ = mc.match_reference(A, B, mc.CONFS["NN-ratio"])
    assert m[11] == -1                                          # s2 == s1: d1 <= 0.64 d2 only if d1 <= 0, and the chain of a unit vector
    sim = mc.sim_chain(A, B)                                    # with itself is not exactly 1 here:
    assert sim[11, 5] == sim[11, 17] == sim[11, 40] and sim[11, 5] < 1
    A2, B2 = mc.tie_case(copies_in_b=False)                     # copies among the rows: column 11's best is row 5, rows 17 and 40 lose
    m, _, _ = mc.match_reference(A2, B2, mc.CONFS["NN-mutual"])
    assert m[5] == 11 and m[17] == -1 and m[40] == -1
    m, _, _ = mc.match_reference(A2, B2, dict(mc.CONFS["NN-mutual"], do_mutual_check=False))
    assert m[5] == m[17] == m[40] == 11


# ---- conf handling ------------------------------------------------------------------------------------------------------------------
def test_conf_names_overrides_and_errors():
    assert set(MATCH_CONFS) == {"NN-mutual", "NN-ratio", "NN-superpoint"} and MATCH_CONFS == mc.CONFS
    assert mc_options(DescriptorMatcher.create("NN-mutual").options()) == dict(ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True)
    assert mc_options(DescriptorMatcher.create("NN-ratio").options()) == dict(ratio_threshold=0.8, distance_threshold=0.0, do_mutual_check=True)
    assert mc_options(DescriptorMatcher.create("NN-superpoint").options()) == dict(ratio_threshold=0.0, distance_threshold=0.7, do_mutual_check=True)
    m = DescriptorMatcher.create({"ratio_threshold": 0.9, "do_mutual_check": False, "max_batch_rows": 100})
    assert m.options() == dict(ratio_threshold=0.9, distance_threshold=None, do_mutual_check=False) and m.conf["max_batch_rows"] == 100
    assert DescriptorMatcher.create().options()["do_mutual_check"] is True
    with pytest.raises(ValueError, match="NN-nope"):
        DescriptorMatcher.create("NN-nope")
    with pytest.raises(ValueError, match="unknown configuration key"):
        DescriptorMatcher.create({"ratio": 0.8})


def test_match_options_struct(tmp_path):
    o = match_options(**MATCH_CONFS["NN-ratio"])
    assert (o.ratio_threshold, o.distance_threshold, o.do_mutual_check, o.reserved) == (0.8, 0.0, 1, 0)
    o = match_options(ratio_threshold=None, distance_threshold=0.7, do_mutual_check=False)
    assert (o.ratio_threshold, o.distance_threshold, o.do_mutual_check, o.reserved) == (0.0, 0.7, 0, 0)
    d = _lib.MatchOptions()
    _lib.load().pxr_match_default_options(ctypes.byref(d))
    assert (d.ratio_threshold, d.distance_threshold, d.do_mutual_check, d.reserved) == (0.0, 0.0, 1, 0)
    src = tmp_path / "sizeof.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pixsfm_hip.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'sizeof(pxr_match_options), offsetof(pxr_match_options, do_mutual_check), offsetof(pxr_match_options, reserved), '
                   'PXR_MATCH_MAX_DIM); return 0; }\n')
    exe = str(tmp_path / "sizeof")
    subprocess.check_call(["gcc", "-I", mc.HERE + "/../include", str(src), "-o", exe])
    want = [ctypes.sizeof(_lib.MatchOptions), _lib.MatchOptions.do_mutual_check.offset, _lib.MatchOptions.reserved.offset, _lib.MATCH_MAX_DIM]
    assert [int(x) for x in subprocess.check_output([exe]).split()] == want and want[0] == 24


# ---- shapes, through the graph ------------------------------------------------------------------------------------------------------
def scene_tracks(owner):
    """The generated tracks: {point id: {(image name, keypoint)}} of the points seen in at least two images."""
    tracks = {}
    for name, ids in owner.items():
        for k, pid in enumerate(ids):
            if pid >= 0:
                tracks.setdefault(int(pid), set()).add((name, k))
    return {p: t for p, t in tracks.items() if len(t) >= 2}


def recovered_tracks(graph, labels):
    out = {}
    for node, lab in zip(graph.nodes, labels):
        out.setdefault(lab, set()).add((graph.image_id_to_name[node.image_id], int(node.feature_idx)))
    return [t for t in out.values() if len(t) >= 2]


def test_match_pairs_feeds_the_graph_and_the_tracks_come_back():
    desc, owner, pairs = mc.scene()
    matcher = ReferenceMatcher.create("NN-ratio")
    matches, scores = matcher.match_pairs(desc, pairs)
    assert len(matches) == len(scores) == len(pairs) == 10
    for (n1, n2), m, s in zip(pairs, matches, scores):
        assert m.dtype == np.uint64 and m.ndim == 2 and m.shape[1] == 2 and s.dtype == np.float32 and s.shape == (len(m),)
        assert len(m) > 0 and (m[:, 0] < len(desc[n1])).all() and (m[:, 1] < len(desc[n2])).all() and ((s > 0.5) & (s <= 1)).all()
        assert (owner[n1][m[:, 0].astype(int)] == owner[n2][m[:, 1].astype(int)]).all()        # every match joins one point's keypoints
    raw = matcher.match_raw(desc, pairs[:2])
    assert raw[0]["matches0"].shape == (len(desc[pairs[0][0]]),) and raw[0]["matches0"].dtype == np.int32
    assert np.array_equal(np.flatnonzero(raw[1]["matches0"] >= 0), matches[1][:, 0].astype(int))
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)
    want = sorted(sorted(t) for t in scene_tracks(owner).values())
    got = sorted(sorted(t) for t in recovered_tracks(graph, labels))
    assert len(want) > 40 and got == want


def test_pairs_2d3d_from_matches_drops_and_orders():
    ids = {"db1": np.array([10, -1, 12, 13]), "db2": np.array([12, 10, -1, 99])}
    matches = [("db1", np.array([[7, 2], [3, 0], [5, 1], [7, 3]], dtype=np.uint64)),       # 7-12, 3-10, 5-none, 7-13
               ("db2", np.array([[3, 1], [7, 0], [2, 3], [3, 3], [9, 2]], dtype=np.uint64))]   # 3-10 (dup), 7-12 (dup), 2-99, 3-99, 9-none
    p2d, p3d = pairs_2d3d_from_matches(matches, ids)
    assert p2d.tolist() == [7, 7, 3, 3, 2] and p3d.tolist() == [12, 13, 10, 99, 99]
    assert p2d.dtype == np.int64 and p3d.dtype == np.int64
    p2d, p3d = pairs_2d3d_from_matches(dict(matches), ids)
    assert p2d.tolist() == [7, 7, 3, 3, 2] and p3d.tolist() == [12, 13, 10, 99, 99]
    p2d, p3d = pairs_2d3d_from_matches({}, ids)
    assert p2d.shape == (0,) and p3d.shape == (0,)
