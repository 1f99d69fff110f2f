"""The source of the retrieval kernels, run lane by lane on the CPU: csrc/pxr_retrieval.hip is compiled as host C++ over the
stand-in runtime of tests/lane_emulation (a fibre per lane, the f32-input MFMA stated as its documented lane maps
and fmaf chain) and held to the reference of tests/retrieval_cases.py bit for bit, like the GPU test does -- the fragment order
and the chunks of the LDS tiles, the masks at the edges, the running best and its butterfly, the validity flags, the integer
atomics across chunks of rows and blocks of centroids, the float64 chains, the rounds of the selection and the host-side
validation are checked without a GPU.  The host's float64 sqrt and division are correctly rounded, as numpy's are; whether the
device's are, and whether the hardware instruction computes the chain, stays with tests/test_retrieval_gpu.py.  Every shape of
that test runs here, the largest selection shape (3, 300, 32768, 20) included (about half a minute of emulated instructions)."""
import ctypes as C

import numpy as np
import pytest

import lanes
import retrieval_cases as rc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "retrieval_on_host.cpp")


def _train(emu, X, K, iters, max_train, dim=None):
    lib, ctx = emu
    X = np.ascontiguousarray(X, np.float32)
    dim = X.shape[1] if dim is None else dim
    cen, cnt, empty = np.full((max(K, 1), max(dim, 1)), -7.0, np.float32), np.full(max(K, 1), -7, np.int32), C.c_int32(-7)
    code = lib.pxr_vocab_train(ctx, C.c_int64(len(X)), C.c_int32(dim), _p(X), C.c_int32(K), C.c_int32(iters), C.c_int64(max_train), _p(cen),
                               _p(cnt), C.byref(empty))
    return code, cen, cnt, empty.value


def _vlad(emu, descs, cen, offsets=None, dim=None, K=None):
    lib, ctx = emu
    cen = np.ascontiguousarray(cen, np.float32)
    K, dim = cen.shape[0] if K is None else K, cen.shape[1] if dim is None else dim
    X = np.ascontiguousarray(np.concatenate(descs), np.float32)
    off = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    G = np.full((len(descs), cen.size), -7.0, np.float32)
    a, n = np.full(len(X), -7, np.int32), np.full((len(descs), cen.shape[0]), -7, np.int32)
    code = lib.pxr_vlad_aggregate(ctx, C.c_int32(len(descs)), _p(off), C.c_int64(len(X)), C.c_int32(dim), _p(X), C.c_int32(K), _p(cen), _p(G),
                                  _p(a), _p(n))
    return code, G, a, n


def _topk(emu, Q, DB, k, query_self=None, mask=None, min_score=None, dim=None):
    lib, ctx = emu
    Q, DB = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(DB, np.float32)
    top, val, found = np.full((len(Q), max(k, 1)), -7, np.int32), np.full((len(Q), max(k, 1)), -7.0, np.float32), np.full(len(Q), -7, np.int32)
    s = None if query_self is None else np.ascontiguousarray(query_self, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    code = lib.pxr_retrieval_topk(ctx, C.c_int32(len(Q)), C.c_int32(len(DB)), C.c_int32(Q.shape[1] if dim is None else dim), _p(Q), _p(DB),
                                  _p(s), _p(m), C.c_int32(k), C.c_double(np.inf if min_score is None else min_score), _p(top), _p(val), _p(found))
    return code, top, val, found


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", rc.ASSIGN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assignment_equals_the_reference(emu, shape):
    X, cen = rc.assignment_case(*shape, seed=300 + rc.ASSIGN_SHAPES.index(shape))
    code, _, a, _ = _vlad(emu, [X], cen)
    lanes.check(emu[0], code)
    ref = rc.assign(X, cen)
    assert np.array_equal(a, ref), np.flatnonzero(a != ref)[:8]
    assert a[0] == 0                                                  # of two identical centroids the lowest index
    if shape[0] >= 4:
        assert a[1] == -1 and a[2] == -1 and a[3] in (shape[1] // 2, 0)


@pytest.mark.parametrize("K,D", [(5, 8), (64, 8), (5, 128), (64, 128)])
def test_aggregation_equals_the_reference(emu, K, D):
    descs, cen = rc.aggregation_case(K, D, seed=40 + K + D)
    code, G, a, n = _vlad(emu, descs, cen)
    lanes.check(emu[0], code)
    rG, ra, rn = rc.vlad(descs, cen)
    assert np.array_equal(a, ra) and np.array_equal(n, rn)
    assert np.array_equal(_bits(G), _bits(rG)), int((_bits(G) != _bits(rG)).sum())
    m = len(rc.AGG_SIZES)
    assert (rn[m] > 0).sum() == 1 and (G[m] != 0).any()               # all rows at one centroid
    assert rn[m + 1].sum() == 1 and not G[m + 1].any()                # one row equal to its centroid: a zero block, nne = 0
    assert rn[m + 2].sum() == 0 and not G[m + 2].any() and not G[0].any()
    # a batch equals its images run alone
    for k in (2, 5, m):
        code, G1, a1, n1 = _vlad(emu, [descs[k]], cen)
        lanes.check(emu[0], code)
        assert np.array_equal(_bits(G1[0]), _bits(G[k])) and np.array_equal(n1[0], n[k])


def test_centroid_blocks_and_row_chunks(emu):
    """K D above the accumulators of one workgroup (blocks of centroids) and an image above one chunk of rows."""
    rng = np.random.default_rng(9)
    cen = rc.unit_rows(rng, 40, 256)
    descs = [rc.clustered_rows(rng, 2100, cen), rc.clustered_rows(rng, 3, cen)]
    code, G, a, n = _vlad(emu, descs, cen)
    lanes.check(emu[0], code)
    rG, ra, rn = rc.vlad(descs, cen)
    assert np.array_equal(a, ra) and np.array_equal(n, rn) and np.array_equal(_bits(G), _bits(rG))


@pytest.mark.parametrize("name", sorted(rc.TRAIN_CASES))
def test_training_equals_the_reference(emu, name):
    X, K, iters, max_train = rc.training_case(name)
    code, cen, cnt, empty = _train(emu, X, K, iters, max_train)
    lanes.check(emu[0], code)
    rcen, rcnt, rempty = rc.vocab_train(X, K, iters, max_train)
    assert np.array_equal(cnt, rcnt) and empty == rempty
    assert np.array_equal(_bits(cen), _bits(rcen)), int((_bits(cen) != _bits(rcen)).sum())
    if name == "duplicates":
        assert empty >= 1 and cnt[4] == 0 and np.array_equal(_bits(cen[4]), _bits(X[2 * len(X) // K]))


@pytest.mark.parametrize("shape", rc.TOPK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_equals_the_reference(emu, shape):
    nq, ndb, dim, k = shape
    rng = np.random.default_rng(700 + dim)
    Q, DB = rc.global_rows(rng, nq, dim), rc.global_rows(rng, ndb, dim)
    got = _topk(emu, Q, DB, k)
    lanes.check(emu[0], got[0])
    ref = rc.topk(Q, DB, k)
    assert np.array_equal(got[1], ref[0]) and np.array_equal(_bits(got[2]), _bits(ref[1])) and np.array_equal(got[3], ref[2])


def test_selection_rules(emu):
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
            got = _topk(emu, DB, DB, k, **kw)
            lanes.check(emu[0], got[0])
            ref = rc.topk(DB, DB, k, **kw)
            assert np.array_equal(got[1], ref[0]), (kw.keys(), k)
            assert np.array_equal(_bits(got[2]), _bits(ref[1])) and np.array_equal(got[3], ref[2])
    top = _topk(emu, DB, DB, 20, query_self=self_, mask=mask)[1]
    assert (top[5] == -1).all() and not (top == self_[:, None]).any() and 4 not in top
    row = top[0].tolist()
    assert row.index(2) + 1 == row.index(6)


def test_bad_input_is_refused_and_leaves_the_outputs_untouched(emu):
    rng = np.random.default_rng(3)
    X = rc.unit_rows(rng, 50, 16)
    cen = rc.unit_rows(rng, 4, 16)
    for kw in (dict(offsets=[1, 20, 50]), dict(offsets=[0, 60, 50]), dict(offsets=[0, 20, 40]), dict(dim=0), dict(dim=513), dict(K=0),
               dict(K=257)):
        code, G, a, n = _vlad(emu, [X[:20], X[20:]], cen, **kw)
        assert code == -1 and (G == -7).all() and (a == -7).all() and (n == -7).all(), kw
    code, G, a, n = _vlad(emu, [rc.unit_rows(rng, 3, 512)], rc.unit_rows(rng, 65, 512))          # K D above 32768
    assert code == -1 and (G == -7).all()
    for args in ((X, 4, -1, 100), (X, 4, 2, 0), (X, 0, 2, 100), (X, 257, 2, 100), (X, 51, 2, 100), (X, 11, 2, 10)):
        code, c, cnt, empty = _train(emu, *args)
        assert code == -1 and (c == -7).all() and (cnt == -7).all() and empty == -7, args[1:]
    code, c, cnt, empty = _train(emu, X, 4, 2, 100, dim=0)
    assert code == -1 and (c == -7).all()
    for kw in (dict(k=0), dict(k=-2), dict(dim=0), dict(dim=32769), dict(min_score=np.nan)):
        k = kw.pop("k", 2)
        code, top, val, found = _topk(emu, X, X, k, **kw)
        assert code == -1 and (top == -7).all() and (val == -7).all() and (found == -7).all(), kw
    with pytest.raises(ValueError, match="pxr_vlad_aggregate.*monotone"):
        lanes.check(emu[0], _vlad(emu, [X[:20], X[20:]], cen, offsets=[0, 60, 50])[0])


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: training on a strided subset, images of different sizes with an empty one and an
    invalid row, the selection with more neighbours asked for than there are."""
    for args in (("5", "40", "24", "6", "3"), ("3", "130", "130", "3", "7"), ("4", "33", "7", "33", "1")):
        stdout = lanes.sanitized(tmp_path, "retrieval_on_host.cpp", "RETRIEVAL_ON_HOST_MAIN", *args)
        w = stdout.split()
        rows, assigned, counted, found = int(w[1]), int(w[3]), int(w[5]), int(w[9])
        assert assigned == rows - 1 and counted == assigned, stdout
        n_images, k = int(args[0]), int(args[4])
        assert 0 < found <= n_images * min(k, n_images - 1), stdout
