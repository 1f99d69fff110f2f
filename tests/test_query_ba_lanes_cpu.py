"""The source of the batched query bundle adjustment, run lane by lane on the CPU: csrc/pxr_query_ba.hip is compiled as host C++
over the stand-in runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the DPP row sums through an exchange
buffer) and held to the oracle's solve of every query like the GPU test does -- the lane groups' blocks at the edges of a
workgroup pass, the ordered sums, the 6 x 6 step, the trust-region decisions and the host-side validation are checked without a
GPU.  What only hardware can show (registers, LDS behaviour, the device's libm) stays with tests/test_query_ba_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import query_ba_cases as qc
from lanes import p as _p

_DT = {np.dtype(np.float16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "query_ba_on_host.cpp")


def _run(emu, full, queries, loss=("cauchy", 0.25), sentinel=False, n_patches=None, upsampling=None, **change):
    """pxr_query_ba_solve on `queries` over the arena of `full` -> per query (summary dict, qvec, tvec).  change: arrays that replace
    the flattened ones; sentinel: return the raw outputs (poses, summaries as bytes) instead, filled with a pattern beforehand."""
    from pixsfm_amd._lib import InterpCfg, LMSummary, Loss, LOSS_IDS
    from pixsfm_amd.engine import lm_options
    lib, ctx = emu
    lib.emu_arena.restype = C.c_void_p
    patches = np.ascontiguousarray(full["patches"])
    corners, scales = np.ascontiguousarray(full["corners"], np.int32), np.ascontiguousarray(full["scales"], np.float64)
    n, H, W, ch = patches.shape
    arena = C.c_void_p(lib.emu_arena(_DT[patches.dtype], ch, H, W, C.c_int64(n if n_patches is None else n_patches), _p(patches), _p(corners),
                                     _p(scales)))
    if upsampling is not None:
        lib.emu_arena_set_upsampling(arena, C.c_double(upsampling))
    f = dict(qc.flatten(queries), cam_model=np.ascontiguousarray(full["cam_model"], np.int32),
             cam_params=np.ascontiguousarray(full["cam_params"], np.float64))
    f.update(change)
    T, N = len(f["query_offsets"]) - 1, len(f["obs_patch"])
    summaries = (LMSummary * max(T, 1))()
    if sentinel:
        C.memset(summaries, 0x5a, C.sizeof(summaries))
    before = (f["qvec"].copy(), f["tvec"].copy(), bytes(summaries))
    cfg, ls, opt = InterpCfg(1, 0, 0), Loss(LOSS_IDS[loss[0]], loss[1]), lm_options()
    rc = lib.pxr_query_ba_solve(ctx, arena, C.c_int32(T), _p(f["query_offsets"]), C.c_int64(N), _p(f["obs_patch"]), _p(f["xyz"]), _p(f["refs"]),
                                _p(f["query_camera"]), C.c_int32(len(f["cam_model"])), _p(f["cam_model"]), _p(f["cam_params"]), _p(f["qvec"]),
                                _p(f["tvec"]), C.byref(cfg), C.byref(ls), C.byref(opt), summaries)
    lib.emu_arena_free(arena)
    if sentinel:
        return rc, before, (f["qvec"], f["tvec"], bytes(summaries))
    lanes.check(lib, rc)
    return [(summaries[i].as_dict(), f["qvec"][i].copy(), f["tvec"][i].copy()) for i in range(T)]


@pytest.fixture(scope="module")
def batch_results(emu):
    return {ch: _run(emu, *qc.boundary_batch(ch)[:2]) for ch in (128, 64)}


@pytest.mark.parametrize("channels", [128, 64])
def test_kernel_source_matches_the_oracle_on_the_boundary_batch(batch_results, channels, capsys):
    """Measured (clang -O1, contraction off), the largest over the queries of both widths: see DESIGN.md section 33."""
    with capsys.disabled():
        qc.compare(batch_results[channels], channels, report="lanes vs oracle, C = %d: " % channels)


def test_trivial_loss_matches_the_oracle(emu):
    full, queries, _ = qc.boundary_batch(128)
    qc.compare(_run(emu, full, queries, loss=("trivial", 1.0)), 128, loss=("trivial", 1.0))


@pytest.mark.parametrize("channels", [128, 64])
def test_a_query_alone_and_the_batch_reversed_give_the_bits_of_the_batch(emu, batch_results, channels):
    full, queries, _ = qc.boundary_batch(channels)
    got = batch_results[channels]
    for i, q in enumerate(queries):
        assert qc.same_bits(_run(emu, full, [q])[0], got[i]), "query at position %d alone" % i
    rev = _run(emu, full, queries[::-1])[::-1]
    for i in range(len(queries)):
        assert qc.same_bits(rev[i], got[i]), "query at position %d in the reversed batch" % i


def test_invalid_arguments_leave_every_output_untouched(emu):
    full, queries, _ = qc.boundary_batch(128)
    queries = [queries[1], queries[5], queries[3]]                  # 1, 0 and 15 blocks
    f = qc.flatten(queries)
    off, N = f["query_offsets"], len(f["obs_patch"])
    bad_patch = f["obs_patch"].copy()
    bad_patch[-1] = len(full["patches"])
    neg_patch = f["obs_patch"].copy()
    neg_patch[0] = -1
    lib = emu[0]
    for change, word in ((dict(query_offsets=np.array([0, 5, off[2], off[3]], np.int64)), "monotone"),
                         (dict(query_offsets=np.array([1, off[1], off[2], off[3]], np.int64)), "not 0"),
                         (dict(query_offsets=np.array([0, off[1], off[2], off[3] - 1], np.int64)), "n_obs"),
                         (dict(query_camera=np.array([0, len(full["cam_model"]), 0], np.int32)), "camera"),
                         (dict(query_camera=np.array([-1, 0, 0], np.int32)), "camera"),
                         (dict(obs_patch=bad_patch), "patch"), (dict(obs_patch=neg_patch), "patch"),
                         (dict(upsampling=2.0), "upsampling")):
        extra = {k: change.pop(k) for k in ("upsampling",) if k in change}
        rc, before, after = _run(emu, full, queries, sentinel=True, **extra, **change)
        assert rc == -1 and word in lib.emu_last_error().decode(), (word, rc, lib.emu_last_error())
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
    # NULL arguments
    from pixsfm_amd._lib import InterpCfg, LMSummary, Loss
    from pixsfm_amd.engine import lm_options
    cfg, ls, opt, s = InterpCfg(1, 0, 0), Loss(1, 0.25), lm_options(), (LMSummary * 3)()
    q, t = f["qvec"].copy(), f["tvec"].copy()
    args = [emu[1], None, C.c_int32(3), _p(off), C.c_int64(N), _p(f["obs_patch"]), _p(f["xyz"]), _p(f["refs"]), _p(f["query_camera"]), C.c_int32(5),
            _p(full["cam_model"]), _p(np.ascontiguousarray(full["cam_params"])), _p(q), _p(t), C.byref(cfg), C.byref(ls), C.byref(opt), s]
    assert lib.pxr_query_ba_solve(*args) == -1 and "NULL" in lib.emu_last_error().decode()
    assert np.array_equal(q, f["qvec"]) and np.array_equal(t, f["tvec"])


def test_unsupported_patches_are_reported_as_such(emu):
    full, queries, _ = qc.boundary_batch(128)
    narrow = dict(full, patches=np.ascontiguousarray(full["patches"][..., :32]))
    q = dict(queries[1], refs=queries[1]["refs"][:, :32])
    rc, before, after = _run(emu, narrow, [q], sentinel=True)
    assert rc == -4 and "not supported" in emu[0].emu_last_error().decode()
    assert before[0].tobytes() == after[0].tobytes() and before[2] == after[2]


def test_a_query_without_a_finite_cost_keeps_its_pose(emu):
    full, queries, _ = qc.boundary_batch(128)
    q = dict(queries[3], xyz=queries[3]["xyz"].copy())
    q["xyz"][2, 1] = np.nan
    (s, qv, tv), (s1, _, _) = _run(emu, full, [q, queries[1]])
    assert s["termination"] == 2 and s["iterations"] == 0 and not np.isfinite(s["initial_cost"])
    assert np.array_equal(qv, q["qvec"]) and np.array_equal(tv, q["tvec"])
    assert s1["termination"] == 0 and s1["final_cost"] < s1["initial_cost"]


def test_sanitized_stand_alone_run(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, every array allocated at
    its exact size: queries of 0, 1, 16 and 17 blocks."""
    out = lanes.sanitized(tmp_path, "query_ba_on_host.cpp", "QUERY_BA_ON_HOST_MAIN", 0, 1, 16, 17)
    lines = out.strip().splitlines()
    assert len(lines) == 4 and all(l.startswith("query %d blocks %d " % (i, n)) for i, (l, n) in enumerate(zip(lines, (0, 1, 16, 17))))
    assert "iterations 0 successful 0 termination 0" in lines[0]
