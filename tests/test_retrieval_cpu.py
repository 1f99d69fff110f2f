"""CPU: the retrieval reference of tests/retrieval_cases.py against a second, independent statement in float64, its defining
properties, and the host side of pixsfm_amd.api.retrieval (the selection itself replaced by the reference: no GPU here)."""
import numpy as np
import pytest

import retrieval_cases as rc


def _vlad64(X, C):
    """VLAD of one image in plain float64: no fixed point, no ordered sums."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    a = np.argmax(X @ C.T, axis=1)
    G = np.zeros_like(C)
    for c in range(len(C)):
        G[c] = (X[a == c] - C[c]).sum(axis=0) if (a == c).any() else 0.0
    norms = np.linalg.norm(G, axis=1)
    nne = (norms > 0).sum()
    G[norms > 0] /= norms[norms > 0, None] * np.sqrt(nne)
    return G.reshape(-1), a


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(21)
    C = rc.unit_rows(rng, 12, 24)
    descs = [rc.clustered_rows(rng, n, C) for n in (80, 3, 150, 41)]
    return descs, C, rc.vlad(descs, C)


def test_float64_statement_agrees_on_tie_free_cases(case):
    descs, C, (G, a, n) = case
    first = 0
    for m, X in enumerate(descs):
        s = np.sort(X.astype(np.float64) @ C.astype(np.float64).T, axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 1e-5                      # tie-free: the two arithmetics must agree on every row
        G64, a64 = _vlad64(X, C)
        assert np.array_equal(a[first:first + len(X)], a64)
        assert np.array_equal(n[m], np.bincount(a64, minlength=len(C)))
        assert np.abs(G[m] - G64).max() < 1e-6
        first += len(X)
    # the vocabulary: one iteration from the same start is the normalised mean of the clusters
    X = np.concatenate(descs)
    cen, cnt, empty = rc.vocab_train(X, 6, 1)
    start = X[[c * len(X) // 6 for c in range(6)]].astype(np.float64)
    a64 = np.argmax(X.astype(np.float64) @ start.T, axis=1)
    assert np.array_equal(cnt, np.bincount(a64, minlength=6)) and empty == (cnt == 0).sum()
    for c in range(6):
        mean = X[a64 == c].astype(np.float64).sum(axis=0)
        assert np.abs(cen[c] - mean / np.linalg.norm(mean)).max() < 1e-6
    # the selection: the float64 order wherever neighbouring similarities are apart
    top, val, found = rc.topk(G, G, 3, query_self=np.arange(len(G), dtype=np.int32))
    sim = G.astype(np.float64) @ G.astype(np.float64).T
    np.fill_diagonal(sim, -np.inf)
    assert np.array_equal(top, np.argsort(-sim, axis=1)[:, :3]) and (found == 3).all()
    assert np.abs(val - np.take_along_axis(sim, top.astype(np.int64), axis=1)).max() < 1e-5


def test_training_is_a_function_of_the_input_alone():
    X, K, iters, max_train = rc.training_case("max_train_below_n")
    a, b = rc.vocab_train(X, K, iters, max_train), rc.vocab_train(X.copy(), K, iters, max_train)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert np.abs(np.linalg.norm(a[0][a[1] > 0], axis=1) - 1).max() < 1e-6
    assert a[1].sum() == max_train and np.array_equal(rc.training_rows(700, 256)[[0, 1, 255]], [0, 2, 697])
    X, K, iters, max_train = rc.training_case("duplicates")
    cen, cnt, empty = rc.vocab_train(X, K, iters, max_train)
    assert empty >= 1 and cnt[4] == 0 and cen[4].tobytes() == X[2 * len(X) // K].tobytes()


def test_defining_properties(case):
    descs, C, (G, a, n) = case
    K, D = C.shape
    rng = np.random.default_rng(5)
    shuffled = [X[rng.permutation(len(X))] for X in descs]
    assert rc.vlad(shuffled, C)[0].tobytes() == G.tobytes()             # integer sums have no order
    for m in range(len(descs)):
        norms = np.linalg.norm(G[m].reshape(K, D).astype(np.float64), axis=1)
        nne = (norms > 0).sum()
        assert nne > 0 and np.abs(norms[norms > 0] - 1 / np.sqrt(nne)).max() < 1e-6
        assert abs(np.linalg.norm(G[m].astype(np.float64)) - 1) < 1e-6
    # invalid rows are assigned -1 and change nothing
    X = descs[0].copy()
    extra = np.concatenate([X, [np.full(D, np.nan, np.float32), np.full(D, 1.5, np.float32)]])
    G2, a2, n2 = rc.vlad([extra], C)
    assert a2[-2:].tolist() == [-1, -1] and G2[0].tobytes() == G[0].tobytes() and np.array_equal(n2[0], n[0])
    # identical images: similarity 1, each other's first neighbour; a query never pairs with itself
    g = {"a": G[0], "b": G[1], "c": G[2], "a_again": G[0].copy(), "d": G[3]}
    pairs = rc.pairs_from_retrieval(g, 2)
    assert pairs[0] == ("a", "a_again") and ("a_again", "a") == [p for p in pairs if p[0] == "a_again"][0]
    assert all(q != d for q, d in pairs) and len(pairs) == 10
    top, val, _ = rc.topk(np.stack(list(g.values())), np.stack(list(g.values())), 1, query_self=np.arange(5, dtype=np.int32))
    assert top[0, 0] == 3 and top[3, 0] == 0 and abs(val[0, 0] - 1) < 1e-5 and abs(val[3, 0] - 1) < 1e-5


def test_selection_rules_of_the_reference():
    rng = np.random.default_rng(12)
    DB = rc.global_rows(rng, 9, 40)
    DB[6] = DB[2]
    DB[4, 3] = np.nan
    mask = np.ones((9, 9), np.uint8)
    mask[5] = 0
    top, val, found = rc.topk(DB, DB, 20, query_self=np.arange(9, dtype=np.int32), mask=mask)
    assert found.tolist() == [7, 7, 7, 7, 0, 0, 7, 7, 7]               # not itself, not the NaN row; the NaN query and the masked one: none
    assert (top[5] == -1).all() and (val[5] == 0).all() and 4 not in top
    row = top[0].tolist()
    assert row.index(2) + 1 == row.index(6) and (top[:, -1] == -1).all()
    cut = rc.topk(DB, DB, 20, min_score=0.05)
    assert cut[2].sum() < rc.topk(DB, DB, 20)[2].sum() and (cut[1][cut[0] >= 0] >= np.float32(0.05)).all()


def test_the_ring_scene_meets_its_condition():
    """What tests/test_retrieval_api_gpu.py relies on: at least 0.9 of the reference's pairs are between images that share at least
    20 points, and their union connects all 24 images."""
    desc, pts = rc.ring_scene()
    names = list(desc)
    cen, _, _ = rc.vocab_train(np.concatenate([desc[n] for n in names]), 16, 10)
    G = rc.vlad([desc[n] for n in names], cen)[0]
    pairs = rc.pairs_from_retrieval(dict(zip(names, G)), 4)
    assert len(pairs) == 24 * 4
    good = sum(len(pts[a] & pts[b]) >= 20 for a, b in pairs)
    assert good >= 0.9 * len(pairs), good
    assert rc.connected(names, pairs)


def test_python_api_host_side(monkeypatch):
    from pixsfm_amd import engine
    from pixsfm_amd.api import retrieval

    def reference_topk(ctx, query, db, num_matched, query_self=None, mask=None, min_score=None, timed=False):
        return rc.topk(query, db, num_matched, query_self, mask, min_score)
    monkeypatch.setattr(engine, "retrieval_topk", reference_topk)
    rng = np.random.default_rng(4)
    g = {"im%d" % k: v for k, v in enumerate(rc.global_rows(rng, 7, 48))}
    names = list(g)
    no_gpu = object()
    assert retrieval.pairs_from_retrieval(g, 3, ctx=no_gpu) == rc.pairs_from_retrieval(g, 3)
    pairs = retrieval.pairs_from_retrieval(g, 3, ctx=no_gpu)
    assert len(pairs) == 21 and [q for q, _ in pairs] == [n for n in names for _ in range(3)] and all(q != d for q, d in pairs)
    q, db = names[:2] + ["im5"], names[2:]
    got = retrieval.pairs_from_retrieval(g, 2, query_names=q, db_names=db, ctx=no_gpu)
    assert got == rc.pairs_from_retrieval(g, 2, q, db) and all(d in db for _, d in got) and ("im5", "im5") not in got
    mask = np.ones((3, 5), bool)
    mask[1] = False
    got = retrieval.pairs_from_retrieval(g, 2, query_names=q, db_names=db, match_mask=mask, min_score=-1.0, ctx=no_gpu)
    assert got == rc.pairs_from_retrieval(g, 2, q, db, -1.0, mask) and not [p for p in got if p[0] == q[1]]
    assert retrieval.pairs_from_retrieval(g, 2, query_names=[], ctx=no_gpu) == []
    with pytest.raises(KeyError):
        retrieval.pairs_from_retrieval(g, 2, query_names=["nowhere"], ctx=no_gpu)
    with pytest.raises(ValueError, match="match_mask"):
        retrieval.pairs_from_retrieval(g, 2, match_mask=np.ones((2, 2), bool), ctx=no_gpu)

    assert retrieval.unique_pairs([("a", "b"), ("b", "a"), ("a", "c"), ("a", "b"), ("c", "b")]) == [("a", "b"), ("a", "c"), ("c", "b")]
    assert retrieval.pairs_from_exhaustive(["a", "b", "c"]) == [("a", "b"), ("a", "c"), ("b", "c")]
    assert retrieval.pairs_from_exhaustive(["q"], ["a", "b"]) == [("q", "a"), ("q", "b")]
    assert len(retrieval.pairs_from_exhaustive(range(9))) == 36

    with pytest.raises(ValueError, match="unknown configuration key"):
        retrieval.GlobalDescriptorExtractor.create({"n_centroids": 4})
    ex = retrieval.GlobalDescriptorExtractor.create({"n_clusters": 4})
    assert ex.conf == {"n_clusters": 4, "n_iterations": 10, "max_train": 262144} and ex.centroids is None
    with pytest.raises(RuntimeError):
        ex.describe({"a": np.zeros((1, 4), np.float32)})
    with pytest.raises(ValueError, match="transpose"):
        ex.fit({"a": np.zeros(4, np.float32)})
    from pixsfm_amd import api
    assert api.pairs_from_retrieval is retrieval.pairs_from_retrieval and api.GlobalDescriptorExtractor is retrieval.GlobalDescriptorExtractor
