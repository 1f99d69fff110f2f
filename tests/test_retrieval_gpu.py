"""GPU: the retrieval kernels (csrc/pxr_retrieval.hip) against the reference of tests/retrieval_cases.py, bit for bit: assign,
counts, n_found and top_index with array_equal, centroids, global descriptors and top_sim as uint32 views.  The reference's
similarity is the float32 fmaf chain and its float64 sqrt and division are numpy's, correctly rounded; that the f32-input MFMA and
the device's float64 sqrt and division give those bits is what these tests establish."""
import ctypes as C

import numpy as np
import pytest

import retrieval_cases as rc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(ref).reshape(-1))
    assert len(bad) == 0, "%s: %d of %d entries differ in bits, first at %s: got %s, reference %s" % (
        what, len(bad), np.size(ref), bad[:4], np.ravel(got)[bad[:4]], np.ravel(ref)[bad[:4]])


def _vlad(ctx, descs, cen):
    from pixsfm_amd.engine import VladVocabulary
    g, a, n = VladVocabulary(ctx, cen).aggregate(list(descs), details=True)
    return g.download(), a.download(), n.download()


def _topk(ctx, Q, DB, k, **kw):
    from pixsfm_amd.engine import retrieval_topk
    return tuple(a.download() for a in retrieval_topk(ctx, Q, DB, k, **kw))


# ---- assignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.ASSIGN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assignment_equals_the_reference(ctx, shape):
    X, cen = rc.assignment_case(*shape, seed=300 + rc.ASSIGN_SHAPES.index(shape))
    a = _vlad(ctx, [X], cen)[1]
    ref = rc.assign(X, cen)
    assert a.dtype == np.int32 and np.array_equal(a, ref), np.flatnonzero(a != ref)[:8]
    assert a[0] == 0                                                  # of two identical centroids the lowest index
    if shape[0] >= 4:
        assert a[1] == -1 and a[2] == -1 and a[3] in (shape[1] // 2, 0)


# ---- aggregation --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aggregation_cases():
    out = {}
    for K, D in ((5, 8), (64, 8), (5, 128), (64, 128)):
        descs, cen = rc.aggregation_case(K, D, seed=40 + K + D)
        out[K, D] = (descs, cen, rc.vlad(descs, cen))
    return out


@pytest.mark.parametrize("K,D", [(5, 8), (64, 8), (5, 128), (64, 128)])
def test_aggregation_equals_the_reference(ctx, aggregation_cases, K, D):
    descs, cen, (rG, ra, rn) = aggregation_cases[K, D]
    G, a, n = _vlad(ctx, descs, cen)
    assert np.array_equal(a, ra) and np.array_equal(n, rn)
    _same_bits(G, rG, "G")
    m = len(rc.AGG_SIZES)
    assert (n[m] > 0).sum() == 1 and G[m].any()                       # all rows at one centroid
    assert n[m + 1].sum() == 1 and not G[m + 1].any()                 # one row equal to its centroid: a zero block, nne = 0
    assert n[m + 2].sum() == 0 and not G[m + 2].any() and not G[0].any()
    # two runs give identical bytes; a batch equals its images run alone
    G2, a2, n2 = _vlad(ctx, descs, cen)
    assert G2.tobytes() == G.tobytes() and a2.tobytes() == a.tobytes() and n2.tobytes() == n.tobytes()
    for k in (2, 5, 6, m):
        G1, _, n1 = _vlad(ctx, [descs[k]], cen)
        assert G1[0].tobytes() == G[k].tobytes() and np.array_equal(n1[0], n[k])


def test_blocks_of_centroids_and_chunks_of_rows(ctx):
    """K D above the accumulators of one workgroup and an image above one chunk of rows."""
    rng = np.random.default_rng(9)
    cen = rc.unit_rows(rng, 40, 256)
    descs = [rc.clustered_rows(rng, 2100, cen), rc.clustered_rows(rng, 3, cen)]
    G, a, n = _vlad(ctx, descs, cen)
    rG, ra, rn = rc.vlad(descs, cen)
    assert np.array_equal(a, ra) and np.array_equal(n, rn)
    _same_bits(G, rG, "G")


# ---- training -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.TRAIN_CASES))
def test_training_equals_the_reference(ctx, name):
    from pixsfm_amd.engine import VladVocabulary
    X, K, iters, max_train = rc.training_case(name)
    voc = VladVocabulary.train(ctx, X, K, iters, max_train)
    cen = voc.centroids
    rcen, rcnt, rempty = rc.vocab_train(X, K, iters, max_train)
    assert np.array_equal(voc.counts, rcnt) and voc.n_empty == rempty
    _same_bits(cen, rcen, "centroids")
    if name == "duplicates":
        assert voc.n_empty >= 1 and voc.counts[4] == 0 and cen[4].tobytes() == X[2 * len(X) // K].tobytes()
    again = VladVocabulary.train(ctx, [X[:len(X) // 3], X[len(X) // 3:]], K, iters, max_train)      # two runs; a list of images
    assert again.centroids.tobytes() == cen.tobytes() and np.array_equal(again.counts, voc.counts)


# ---- selection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.TOPK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_equals_the_reference(ctx, shape):
    nq, ndb, dim, k = shape
    rng = np.random.default_rng(700 + dim)
    Q, DB = rc.global_rows(rng, nq, dim), rc.global_rows(rng, ndb, dim)
    top, val, found = _topk(ctx, Q, DB, k)
    rtop, rval, rfound = rc.topk(Q, DB, k)
    assert np.array_equal(top, rtop) and np.array_equal(found, rfound)
    _same_bits(val, rval, "top_sim")
    again = _topk(ctx, Q, DB, k)
    assert again[0].tobytes() == top.tobytes() and again[1].tobytes() == val.tobytes()


def test_selection_rules(ctx):
    rng = np.random.default_rng(12)
    DB = rc.global_rows(rng, 9, 40)
    DB[6] = DB[2]                                                      # two identical rows: the index decides
    DB[4, 3] = np.nan                                                  # a NaN row is never a candidate
    self_ = np.arange(9, dtype=np.int32)
    mask = np.ones((9, 9), np.uint8)
    mask[5] = 0                                                        # a row that excludes everything
    mask[0, 1] = 0
    for kw in (dict(), dict(query_self=self_), dict(query_self=self_, mask=mask), dict(query_self=self_, min_score=0.05),
               dict(min_score=-0.1, mask=mask)):
        for k in (1, 3, 20):                                           # 20 > candidates: padding
            top, val, found = _topk(ctx, DB, DB, k, **kw)
            rtop, rval, rfound = rc.topk(DB, DB, k, **kw)
            assert np.array_equal(top, rtop), (sorted(kw), k)
            assert np.array_equal(found, rfound)
            _same_bits(val, rval, "top_sim")
    assert rc.topk(DB, DB, 20, query_self=self_, min_score=0.05)[2].sum() < rc.topk(DB, DB, 20, query_self=self_)[2].sum()   # it cuts
    top = _topk(ctx, DB, DB, 20, query_self=self_, mask=mask)[0]
    assert (top[5] == -1).all() and not (top == self_[:, None]).any() and 4 not in top
    row = top[0].tolist()
    assert row.index(2) + 1 == row.index(6)


# ---- bad input ----------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_and_leaves_the_outputs_untouched(ctx):
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(3)
    X, cen = rc.unit_rows(rng, 50, 16), rc.unit_rows(rng, 4, 16)
    d_x, d_c = ctx.to_device(X, np.float32), ctx.to_device(cen, np.float32)
    sentinel = lambda shape, dt: ctx.to_device(np.full(shape, -7, dt), dt)       # noqa: E731
    untouched = lambda *arrays: all((a.download() == -7).all() for a in arrays)  # noqa: E731

    def aggregate(offsets=(0, 20, 50), n_total=50, dim=16, K=4):
        g, a, n = sentinel((2, 64), np.float32), sentinel((50,), np.int32), sentinel((2, 4), np.int32)
        d_off = ctx.to_device(np.asarray(offsets, np.int64), np.int64)
        code = lib.pxr_vlad_aggregate(h, 2, d_off.ptr, n_total, dim, d_x.ptr, K, d_c.ptr, g.ptr, a.ptr, n.ptr)
        ctx.sync()
        return code, untouched(g, a, n)

    assert aggregate()[0] == 0
    for kw in (dict(offsets=(1, 20, 50)), dict(offsets=(0, 60, 50)), dict(offsets=(0, 20, 40)), dict(dim=0), dict(dim=513), dict(K=0),
               dict(K=257), dict(dim=512, K=65), dict(n_total=-1), dict(n_total=1 << 30)):
        assert aggregate(**kw) == (-1, True), kw

    def train(n_total=50, dim=16, K=4, iters=2, max_train=100):
        c, cnt, empty = sentinel((4, 16), np.float32), sentinel((4,), np.int32), C.c_int32(-7)
        code = lib.pxr_vocab_train(h, n_total, dim, d_x.ptr, K, iters, max_train, c.ptr, cnt.ptr, C.byref(empty))
        ctx.sync()
        return code, untouched(c, cnt) and empty.value == -7

    assert train()[0] == 0
    for kw in (dict(iters=-1), dict(max_train=0), dict(K=0), dict(K=257), dict(K=51), dict(K=4, max_train=3), dict(dim=0), dict(dim=513),
               dict(n_total=-1), dict(n_total=1 << 30), dict(dim=512, K=65)):
        assert train(**kw) == (-1, True), kw

    def select(dim=16, k=2, min_score=np.inf):
        top, val, found = sentinel((50, 2), np.int32), sentinel((50, 2), np.float32), sentinel((50,), np.int32)
        code = lib.pxr_retrieval_topk(h, 50, 50, dim, d_x.ptr, d_x.ptr, None, None, k, float(min_score), top.ptr, val.ptr, found.ptr)
        ctx.sync()
        return code, untouched(top, val, found)

    assert select()[0] == 0
    for kw in (dict(k=0), dict(k=-3), dict(dim=0), dict(dim=32769), dict(min_score=np.nan)):
        assert select(**kw) == (-1, True), kw
    from pixsfm_amd._lib import PixsfmHipError
    from pixsfm_amd.engine import VladVocabulary
    with pytest.raises(PixsfmHipError, match="pxr_vocab_train.*n_clusters"):
        VladVocabulary.train(ctx, X, 51)


def test_timed_twins_report_every_kernel(ctx):
    from pixsfm_amd.engine import VladVocabulary, retrieval_topk
    X, K, iters, max_train = rc.training_case("max_train_below_n")
    voc = VladVocabulary.train(ctx, X, K, iters, max_train, timed=True)
    assert sorted(voc.kernel_ms) == ["accumulate", "assign", "gather", "update"] and all(v > 0 for v in voc.kernel_ms.values())
    plain = VladVocabulary.train(ctx, X, K, iters, max_train)
    assert plain.centroids.tobytes() == voc.centroids.tobytes()
    g = voc.aggregate([X[:100], X[100:]], timed=True)
    assert sorted(voc.kernel_ms) == ["accumulate", "assign", "finalise"] and all(v > 0 for v in voc.kernel_ms.values())
    assert voc.aggregate([X[:100], X[100:]]).download().tobytes() == g.download().tobytes()
    ms = retrieval_topk(ctx, g, g, 1, timed=True)[3]
    assert sorted(ms) == ["select", "similarity"] and all(v > 0 for v in ms.values())
