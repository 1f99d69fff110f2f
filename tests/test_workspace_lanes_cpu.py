"""The typed workspace layout of csrc/pxr_batch.h (Workspace) and the one grow of csrc/pxr_internal.h (grow_block), on their own on
the CPU over the stand-in runtime of tests/lane_emulation: every array starts at the next multiple of 256 bytes in the order it
was taken, a count of 0 takes no room, the pointers are filled only by the commit, the block grows only when it must, and a failed
hipMalloc releases the context's caches only where the caller allows it.  The expected offsets are computed here from
(count * sizeof(T) + 255) & ~255; the layout class is not asked for them."""
import ctypes as C

import numpy as np
import pytest

import lanes
from lanes import p as _p

PXR_EHIP = -2
# the kinds of tests/lane_emulation/workspace_on_host.cpp: uint8_t, const uint8_t, int32_t, const int32_t, double, const double,
# a 24-byte struct, the same const -- all struct members
ELEM = (1, 1, 4, 4, 8, 8, 24, 24)
# (kind, count): a count of 0 in first, middle and last place; 32 doubles and 32 structs are 256 and 768 bytes exactly; the others
# end inside a 256-byte unit, one of them (257 bytes) just past its start
ARRAYS = ((0, 0), (4, 32), (1, 1), (2, 63), (3, 65), (5, 0), (6, 7), (7, 32), (0, 257), (5, 1000), (4, 3), (2, 0))


def _expected(arrays):
    """(the offset of every array, the total) by the rule, independent of the class."""
    offsets, at = [], 0
    for kind, count in arrays:
        offsets.append(at)
        at += (count * ELEM[kind] + 255) & ~255
    return offsets, at


@pytest.fixture()
def emu(tmp_path_factory):
    lib, _ = lanes.load(tmp_path_factory, "workspace_on_host.cpp")
    lib.emu_ctx.restype = C.c_void_p
    ctx = C.c_void_p(lib.emu_ctx())                         # a context of its own per test: each starts without a workspace
    yield lib, ctx
    lib.emu_ctx_free(ctx)


def _layout(lib, ctx, arrays):
    kinds = np.array([k for k, _ in arrays], np.int32)
    counts = np.array([c for _, c in arrays], np.int64)
    offsets = np.full(len(arrays), -7, np.int64)
    info = np.full(3, -7, np.int64)
    lanes.check(lib, lib.emu_ws_layout(ctx, len(arrays), _p(kinds), _p(counts), _p(offsets), _p(info)))
    return offsets.tolist(), dict(moved=int(info[0]), mallocs=int(info[1]), bytes=int(info[2]))


def test_the_list_covers_what_it_should():
    assert {ELEM[k] for k, _ in ARRAYS} == {1, 4, 8, 24} and set(range(8)) == {k for k, _ in ARRAYS}
    assert ARRAYS[0][1] == 0 and ARRAYS[-1][1] == 0 and any(c == 0 for _, c in ARRAYS[1:-1])
    assert any(c > 0 and c * ELEM[k] % 256 == 0 for k, c in ARRAYS)


def test_every_pointer_is_base_plus_the_expected_offset(emu):
    lib, ctx = emu
    offsets, info = _layout(lib, ctx, ARRAYS)
    expect, total = _expected(ARRAYS)
    assert offsets == expect                                 # const and non-const members alike; none left unfilled (-1)
    assert info == dict(moved=1, mallocs=1, bytes=total)


def test_a_commit_that_fits_does_not_reallocate_and_a_larger_one_does_once(emu):
    lib, ctx = emu
    _, first = _layout(lib, ctx, ARRAYS)
    offsets, again = _layout(lib, ctx, ARRAYS)
    assert offsets == _expected(ARRAYS)[0] and again == dict(moved=0, mallocs=0, bytes=first["bytes"])
    half = ARRAYS[2:7]                                       # a second, smaller layout on the same context starts again at offset 0
    offsets, info = _layout(lib, ctx, half)
    assert offsets == _expected(half)[0] and offsets[0] == 0 and info == dict(moved=0, mallocs=0, bytes=first["bytes"])
    larger = tuple((k, 3 * c) for k, c in ARRAYS)
    offsets, info = _layout(lib, ctx, larger)
    expect, total = _expected(larger)
    assert total > first["bytes"] and offsets == expect and info["mallocs"] == 1 and info["bytes"] == total


@pytest.mark.parametrize("release", (1, 0))
def test_a_failed_allocation_releases_the_caches_only_when_allowed(emu, release):
    lib, ctx = emu
    out = np.full(8, -7, np.int64)
    lanes.check(lib, lib.emu_ws_fail_once(ctx, release, C.c_int64(1000), _p(out)))
    rc, gram_null, gram_bytes, arena_null, arena_bytes, ws_bytes, mallocs, filled = out.tolist()
    if release:                                              # both caches freed and zeroed, the retry succeeds
        assert (rc, gram_null, gram_bytes, arena_null, arena_bytes, ws_bytes, mallocs, filled) == (0, 1, 0, 1, 0, 1024, 2, 1)
    else:                                                    # PXR_EHIP, both caches left alone, nothing handed out
        assert (rc, gram_null, gram_bytes, arena_null, arena_bytes, ws_bytes, mallocs, filled) == (PXR_EHIP, 0, 64, 0, 64, 0, 1, 0)


def test_sanitized_stand_alone_program(tmp_path):
    """The same list, the list again, its first half, the list tripled and the two failure cases with a main of their own under
    AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: the block has the layout's exact size and every
    array is written from its first to its last byte, so an offset or a total that is too small is caught."""
    stdout = lanes.sanitized(tmp_path, "workspace_on_host.cpp", "WORKSPACE_ON_HOST_MAIN", *("%d:%d" % a for a in ARRAYS))
    lines = [ln.split() for ln in stdout.strip().splitlines()]
    half, tripled = ARRAYS[:len(ARRAYS) // 2], tuple((k, 3 * c) for k, c in ARRAYS)
    total = _expected(ARRAYS)[1]
    runs = (("first", ARRAYS, 1, 1, total), ("again", ARRAYS, 0, 0, total), ("half", half, 0, 0, total),
            ("tripled", tripled, None, 1, _expected(tripled)[1]))   # (a new block may get the old one's address: not asserted)
    for words, (name, arrays, moved, mallocs, nbytes) in zip(lines, runs):
        assert words[0] == name and words[3:8] == ["mallocs", str(mallocs), "bytes", str(nbytes), "offsets"], stdout
        assert words[1] == "moved" and (moved is None or words[2] == str(moved)), stdout
        assert [int(w) for w in words[8:]] == _expected(arrays)[0], stdout
    grown = (_expected(tripled)[1] + 1000 + 255) & ~255
    assert lines[4] == ["release", "1:"] + [str(v) for v in (0, 1, 0, 1, 0, grown, 2, 1)], stdout
    assert lines[5] == ["release", "0:"] + [str(v) for v in (PXR_EHIP, 0, 64, 0, 64, 0, 1, 0)], stdout
    assert len(lines) == 6, stdout
