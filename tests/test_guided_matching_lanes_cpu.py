"""The source of the guided matching kernels, run lane by lane on the CPU: csrc/pxr_match.hip compiled as host C++ over the
stand-in runtime of tests/lane_emulation (as tests/test_matching_lanes_cpu.py does for the unguided entry point) and held
to the reference of tests/guided_matching_cases.py bit for bit -- the records, the gate in the tile loop's epilogue on both the
row and the column side, the LDS row records at the strip edges, the host-side validation -- without a GPU.  The same translation
unit runs once more with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program."""
import ctypes as C

import numpy as np
import pytest

import guided_matching_cases as gc
import lanes
import matching_cases as mc
from lanes import p as _p
from test_matching_lanes_cpu import _equal

SHAPES = [(1, 1, 4), (1, 37, 128), (37, 1, 128), (33, 31, 128), (129, 65, 128), (70, 90, 130)]
SENTINEL = -7


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "match_on_host.cpp")          # the build that tests/test_matching_lanes_cpu.py uses


def guided_call(call, descs, xy, pairs, kinds, models, thrs, offsets=None, dim=None, null=(), reserved=0, **options):
    """One call of pxr_match_guided over host or device arrays: `call(args...) -> rc` gets the arrays.  Returns (rc, matches0,
    scores0, n_matches), the outputs filled with SENTINEL before the call.  null: the names among "xy", "kinds", "models", "thrs"
    that go in as NULL pointers; reserved: options.reserved."""
    from pixsfm_amd.engine import match_options
    dim = descs[0].shape[1] if dim is None else dim
    desc = np.ascontiguousarray(np.concatenate(descs), np.float32)
    kp = np.ascontiguousarray(np.concatenate(xy), np.float64).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    sizes = [len(descs[a]) if 0 <= a < len(descs) else 0 for a, _ in pairs]
    poff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kinds, thrs = np.ascontiguousarray(kinds, np.int32), np.ascontiguousarray(thrs, np.float64)
    models = np.ascontiguousarray(models, np.float64).reshape(-1, 9)
    m, s, n = np.full(poff[-1], SENTINEL, np.int32), np.full(poff[-1], SENTINEL, np.float32), np.full(len(pairs), SENTINEL, np.int32)
    opts = match_options(**options)
    opts.reserved = reserved
    kp, kinds, models, thrs = (None if name in null else a for name, a in (("xy", kp), ("kinds", kinds), ("models", models), ("thrs", thrs)))
    rc = call(C.c_int32(len(descs)), off, C.c_int64(len(desc)), C.c_int32(dim), desc, kp, C.c_int32(len(pairs)), pairs, poff, kinds,
              models, thrs, opts, m, s, n)
    return rc, m, s, n


def _run(emu, *args, **kw):
    lib, ctx = emu

    def call(n_images, off, n_total, dim, desc, kp, n_pairs, pairs, poff, kinds, models, thrs, opts, m, s, n):
        return lib.pxr_match_guided(ctx, n_images, _p(off), n_total, dim, _p(desc), _p(kp), n_pairs, _p(pairs), _p(poff), _p(kinds),
                                    _p(models), _p(thrs), C.byref(opts), _p(m), _p(s), _p(n))
    rc, m, s, n = guided_call(call, *args, **kw)
    if rc:
        assert (m == SENTINEL).all() and (s == SENTINEL).all() and (n == SENTINEL).all(), "an error wrote to the outputs"
    lanes.check(lib, rc)
    return m, s, n


def _run_case(emu, c, **options):
    return _run(emu, [c["A"], c["B"]], [c["xy_a"], c["xy_b"]], [(0, 1)], [c["kind"]], [c["M"]], [c["thr"]], **options)


def _reference(c, **options):
    rm, rs, rn = gc.guided_reference(c["A"], c["B"], c["xy_a"], c["xy_b"], c["kind"], c["M"], c["thr"], **options)
    return rm, rs, np.array([rn], np.int32)


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_source_equals_the_reference(emu, shape, kind):
    c = gc.gated_pair(*shape, gc.KINDS[kind], seed=200 + SHAPES.index(shape))
    for name, options in mc.OPTION_SETS.items():
        _equal(_run_case(emu, c, **options), _reference(c, **options), "%s %s %s" % (shape, kind, name))


@pytest.mark.parametrize("kind", sorted(gc.KINDS))
def test_planted_rows_and_columns(emu, kind):
    c = gc.edge_pair(gc.KINDS[kind])
    gc.check_edge_pair(c, lambda case, **o: _run_case(emu, case, **o))
    for name, options in mc.OPTION_SETS.items():
        _equal(_run_case(emu, c, **options), _reference(c, **options), "edge %s %s" % (kind, name))


def test_the_batch(emu):
    descs, xy, pairs, kinds, models, thrs = gc.gated_batch()
    for name, options in mc.OPTION_SETS.items():
        ref = gc.reference_batch(descs, xy, pairs, kinds, models, thrs, options)
        _equal(_run(emu, descs, xy, pairs, kinds, models, thrs, **options), ref, "batch " + name)
    assert ref[2][-1] == 0


def invalid_calls():
    """(keyword changes of a valid two-image call, a word of the error text): every class of PXR_EINVAL."""
    return ((dict(offsets=[1, 40, 90]), "d_image_offsets"), (dict(offsets=[0, 95, 90]), "monotone"), (dict(offsets=[0, 40, 80]), "n_total"),
            (dict(pairs=[(0, 1), (1, 2)]), "d_pairs"), (dict(dim=0), "dim"), (dict(dim=513), "dim"),
            (dict(kinds=[0, 2]), "d_pair_kind"), (dict(kinds=[-1, 1]), "d_pair_kind"), (dict(thrs=[0.1, -0.5]), "d_pair_thr"),
            (dict(thrs=[np.nan, 0.1]), "d_pair_thr"), (dict(ratio_threshold=np.inf), "threshold"), (dict(distance_threshold=np.nan), "threshold"),
            (dict(null=("xy",)), "NULL d_xy"), (dict(null=("kinds",)), "NULL d_pair_kind"), (dict(null=("models",)), "NULL d_pair_kind"),
            (dict(null=("thrs",)), "NULL d_pair_kind"), (dict(reserved=1), "reserved"))


def valid_call():
    rng = np.random.default_rng(8)
    descs = [mc.unit_rows(rng, n, 16) for n in (40, 50)]
    xy = [rng.uniform(-1, 1, (len(d), 2)) for d in descs]
    return dict(descs=descs, xy=xy, pairs=[(0, 1), (1, 0)], kinds=[0, 1], models=[gc.random_model(rng, 0), gc.random_model(rng, 1)],
                thrs=[0.3, np.inf])


def test_validation(emu):
    for change, word in invalid_calls():
        kw = valid_call()
        kw.update(change)
        with pytest.raises(ValueError, match="pxr_match_guided.*" + word):        # _run checks that every output byte kept its sentinel
            _run(emu, **kw)
    m, s, n = _run(emu, **valid_call())
    assert (m != SENTINEL).all() and (n >= 0).all()
    kw = valid_call()
    kw.update(descs=[d[:0] for d in kw["descs"]], xy=[k[:0] for k in kw["xy"]])
    m, s, n = _run(emu, **kw)
    assert len(m) == 0 and n.tolist() == [0, 0]


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: (1, 1, 1), (129, 65, 128) and the batch with the empty images, both kinds."""
    stdout = lanes.sanitized(tmp_path, "guided_on_host.cpp", "GUIDED_ON_HOST_MAIN")
    lines = stdout.strip().split("\n")
    assert len(lines) == 3 and all("error" not in ln for ln in lines), stdout
    counts = [int(w) for w in lines[2].split(":")[1].split()]
    assert lines[2].startswith("batch") and len(counts) == 7, stdout
    assert counts[4:6] == [0, 0] and counts[0] > 0, stdout          # an empty image on either side; (4, 4) under E keeps some
