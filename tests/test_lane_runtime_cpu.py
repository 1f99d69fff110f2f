"""The stand-in runtime of the lane emulation (tests/lane_emulation/hip/hip_runtime.h) held to what its header says of it, one
primitive at a time against plain numpy: tests/lane_emulation/runtime_on_host.cpp has one small kernel per primitive.  The
stages' tests (tests/test_*_lanes_cpu.py) rely on these; what the hardware does is the business of the GPU tests."""
import numpy as np
import pytest

import lanes
from lanes import p as _p

GRID, BLOCK = 2, 256


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "runtime_on_host.cpp")


def _lane():
    return np.arange(GRID * BLOCK)


@pytest.mark.parametrize("width", [16, 64])
def test_shuffles(emu, width):
    rng = np.random.default_rng(width)
    lane, n = _lane(), GRID * BLOCK
    v, src, mask = rng.normal(size=n), rng.integers(0, 200, n).astype(np.int32), 5
    picked, swapped = np.full(n, -7.0), np.full(n, -7.0)
    emu[0].emu_shuffles(GRID, BLOCK, _p(v), _p(src), mask, width, _p(picked), _p(swapped))
    base = lane - lane % width                                        # a source is taken modulo the width, inside the lane's own segment
    assert np.array_equal(picked, v[base + src % width])
    assert np.array_equal(swapped, v[base + (lane % width ^ mask)])


def test_row_sums(emu):
    """row16_sum and row8_sum of pxr_device.h over the DPP stand-in: every lane holds the sum of its 16 or 8 lanes, added in the
    order of the four (three) permutations, bit for bit."""
    lane, n = _lane(), GRID * BLOCK
    v = np.random.default_rng(3).normal(size=n)
    sum16, sum8 = np.full(n, -7.0), np.full(n, -7.0)
    emu[0].emu_row_sums(GRID, BLOCK, _p(v), _p(sum16), _p(sum8))
    row, l = lane - lane % 16, lane % 16
    s = v.copy()
    for step, from_ in enumerate((l ^ 1, l ^ 2, (l & 8) | (7 - (l & 7)), 15 - l)):
        s = s + s[row + from_]
        if step == 2:
            assert np.array_equal(sum8, s)
    assert np.array_equal(sum16, s)
    assert np.allclose(sum16, v.reshape(-1, 16).sum(1).repeat(16), rtol=0, atol=1e-14)
    assert np.allclose(sum8, v.reshape(-1, 8).sum(1).repeat(8), rtol=0, atol=1e-14)


@pytest.mark.parametrize("block", [64, 96])
def test_ballot(emu, block):
    """The bitmask of the predicate over the caller's wavefront; at 96 the second wavefront has 32 lanes."""
    pred = np.random.default_rng(block).integers(0, 2, GRID * block).astype(np.int32) * 3          # any non-zero value is true
    mask = np.full(GRID * block, 7, np.uint64)
    emu[0].emu_ballot(GRID, block, _p(pred), _p(mask))
    for g in range(GRID):
        for wave in range(0, block, 64):
            bits = pred[g * block + wave:g * block + min(wave + 64, block)] != 0
            want = sum(1 << i for i in np.flatnonzero(bits))
            assert (mask[g * block + wave:g * block + min(wave + 64, block)] == np.uint64(want)).all(), (g, wave)
            assert bits.any() and not bits.all()


def test_syncthreads_count(emu):
    pred = (np.random.default_rng(4).integers(0, 3, GRID * BLOCK) == 0).astype(np.int32) * 5
    count = np.full(GRID * BLOCK, -7, np.int32)
    emu[0].emu_count(GRID, BLOCK, _p(pred), _p(count))
    want = (pred.reshape(GRID, BLOCK) != 0).sum(1)
    assert want[0] != want[1] and np.array_equal(count, want.repeat(BLOCK))


def _fmaf(a, b, c):
    """float32 fmaf in numpy.  The float64 product of two float32 is exact; the float64 sum is rounded to odd with its error term
    (TwoSum), after which the rounding to float32 is the only one that counts."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                                       # p + c = s + e exactly
    odd = np.where((e != 0) & (s.view(np.int64) & 1 == 0), np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(np.float32)


@pytest.mark.parametrize("K", [2, 6])
def test_mfma_stand_in_is_the_k_ordered_fmaf_chain(emu, K):
    rng = np.random.default_rng(K)
    A, B, Cm = (rng.normal(size=s).astype(np.float32) for s in ((32, K), (K, 32), (32, 32)))
    D = np.full((32, 32), -7.0, np.float32)
    emu[0].emu_mfma(_p(A), _p(B), _p(Cm), K, _p(D))
    want = Cm.copy()
    for k in range(K):                                                # for every (i, j): want[i][j] = fmaf(A[i][k], B[k][j], want[i][j])
        want = _fmaf(A[:, k:k + 1], B[k:k + 1, :], want)
    assert np.array_equal(D.view(np.uint32), want.view(np.uint32))


def test_atomic_cas_hits_and_misses(emu):
    n = GRID * 64
    slot = np.arange(n, dtype=np.uint64) * np.uint64(2 ** 40 + 1)
    expected = slot.copy()
    expected[1::3] += np.uint64(1)                                    # every third lane misses
    desired, was, before = slot + np.uint64(99), np.full(n, 7, np.uint64), slot.copy()
    emu[0].emu_cas(GRID, 64, _p(slot), _p(expected), _p(desired), _p(was))
    assert np.array_equal(was, before)
    assert np.array_equal(slot, np.where(expected == before, desired, before))


def test_a_launch_reaches_every_lane_of_every_block(emu):
    n = GRID * BLOCK
    block, thread, dim = (np.full(n, -7, np.int32) for _ in range(3))
    emu[0].emu_indices(GRID, BLOCK, _p(block), _p(thread), _p(dim))
    assert np.array_equal(block, _lane() // BLOCK) and np.array_equal(thread, _lane() % BLOCK) and (dim == BLOCK).all()


def test_groups_on_paths_of_their_own_stay_in_lockstep(emu):
    """The lockstep rule of the header: 16-lane groups that run different numbers of cross-lane calls, or return at once, get
    their own group's values."""
    n = GRID * BLOCK
    v = np.random.default_rng(6).integers(-50, 50, n).astype(np.float64)      # small integers: every order of the sums is exact
    out = np.full(n, -7.0)
    emu[0].emu_groups(GRID, BLOCK, _p(v), _p(out))
    group = _lane() % BLOCK // 16
    want = v.reshape(-1, 16).sum(1).repeat(16) * 16.0 ** (group % 3)
    assert np.array_equal(out, np.where(group % 4 == 3, -1.0, want))
