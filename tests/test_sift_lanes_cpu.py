"""The source of the SIFT kernels, run lane by lane on the CPU: csrc/pxr_sift.hip is compiled as host C++ over the stand-in
runtime of tests/lane_emulation (a fibre per lane, workgroup-wide barriers, the 64-lane shuffles through an exchange
buffer) and held to the numpy reference of tests/sift_cases.py on small shapes: the tiles and halos of the blur at the edges of
a level, the count / scan / write of the detection across wavefronts, chunks and blocks, the owner-computes histograms, the
host-side validation.  The arithmetic here is the host's float32 and float64, so the pyramid is held to the derived bound of
sift_cases.pass_bound and everything after it to the reference run on the emulation's own pyramid, where only the order of a few
float64 sums differs.  What only hardware can show stays with tests/test_sift_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import lanes
import sift_cases as sc
from lanes import p as _p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lanes.load(tmp_path_factory, "sift_on_host.cpp")


def _options(**kw):
    from pixsfm_amd import _lib
    o = _lib.SiftOptions()
    for k, v in sc.DEFAULTS.items():
        setattr(o, k, kw.get(k, v))
    return o


def _pyramid(emu, image, **kw):
    """The emulation's pyramid as [octave: (S + 3, h, w) float32], through the layout the library reports."""
    lib, ctx = emu
    o = _options(**kw)
    h, w = image.shape
    n_oct, sizes, offs, nbytes = C.c_int32(-1), np.zeros((8, 2), np.int32), np.zeros(8, np.int64), C.c_int64(-1)
    lanes.check(lib, lib.pxr_sift_pyramid_layout(h, w, C.byref(o), C.byref(n_oct), _p(sizes), _p(offs)))
    lanes.check(lib, lib.pxr_sift_pyramid_bytes(h, w, C.byref(o), C.byref(nbytes)))
    flat = np.full(nbytes.value // 4, -7.0, np.float32)
    img = np.ascontiguousarray(image)
    lanes.check(lib, lib.pxr_sift_pyramid(ctx, _p(img), 3 if img.dtype == np.uint8 else 1, h, w, C.byref(o), _p(flat)))
    S = o.octave_resolution
    levels = [flat[offs[k]:offs[k] + (S + 3) * sizes[k, 0] * sizes[k, 1]].reshape(S + 3, sizes[k, 0], sizes[k, 1]) for k in range(n_oct.value)]
    assert sum(lv.size for lv in levels) == flat.size
    return flat, levels, o


def _detect(emu, flat, h, w, o, capacity):
    lib, ctx = emu
    kp, rec, resp = np.full((capacity, 4), -9.0), np.full((capacity, 4), -9, np.int32), np.full(capacity, -9.0, np.float32)
    found = C.c_int64(-9)
    lanes.check(lib, lib.pxr_sift_detect(ctx, _p(flat), h, w, C.byref(o), C.c_int64(capacity), _p(kp), _p(rec), _p(resp), C.byref(found)))
    return kp, rec, resp, found.value


def _describe(emu, flat, h, w, o, kp):
    lib, ctx = emu
    kp = np.ascontiguousarray(kp, np.float64).reshape(-1, 4)
    desc, valid = np.full((len(kp), 128), -9.0, np.float32), np.full(len(kp), 9, np.uint8)
    lanes.check(lib, lib.pxr_sift_describe(ctx, _p(flat), h, w, C.byref(o), C.c_int64(len(kp)), _p(kp), _p(desc), _p(valid)))
    return desc, valid


CASES = [("blobs_17x23", lambda: sc.blob_image(17, 23, [(11.3, 8.6, 2.0, 0.4)]), dict()),
         ("texture_65x63_u8", lambda: sc.textured_image(65, 63, 3), dict()),
         ("texture_64x64_octave0", lambda: sc.textured_image(64, 64, 4), dict(first_octave=0)),
         ("texture_33x70_S2_upright_L2", lambda: sc.textured_image(33, 70, 5), dict(octave_resolution=2, upright=1, normalization=0, first_octave=0)),
         ("texture_40x37_S4_four_orientations", lambda: sc.textured_image(40, 37, 6), dict(octave_resolution=4, max_num_orientations=4, first_octave=0))]


@pytest.mark.parametrize("name,make,kw", CASES, ids=[c[0] for c in CASES])
def test_kernel_source_matches_the_reference(emu, name, make, kw):
    image = make()
    h, w = image.shape
    opt = sc.options(**kw)
    flat, levels, o = _pyramid(emu, image, **kw)
    ref = sc.pyramid(image, opt)
    bound = sc.pass_bound(image, opt)
    assert len(levels) == len(ref)
    for k in range(len(ref)):
        assert levels[k].shape == ref[k].shape
        for s in range(len(ref[k])):
            assert np.abs(levels[k][s] - ref[k][s]).max() <= bound[k][s], (k, s)
    # from here on the reference runs on the emulation's own float32 pyramid: the same decisions, the same numbers
    own = [lv.astype(np.float64) for lv in levels]
    f = sc.features(own, opt)
    n = len(f["keypoints"])
    assert n > 0
    kp, rec, resp, found = _detect(emu, flat, h, w, o, n + 3)
    assert found == n
    assert np.array_equal(rec[:n], f["record"])
    assert (kp[n:] == -9).all() and (rec[n:] == -9).all() and (resp[n:] == -9).all()
    assert np.abs(kp[:n] - f["keypoints"]).max() <= 1e-9
    assert np.abs(resp[:n] - f["response"]).max() <= 1e-7
    d_ref, v_ref = sc.describe(own, opt, kp[:n])
    desc, valid = _describe(emu, flat, h, w, o, kp[:n])
    assert np.array_equal(valid.astype(bool), v_ref)
    assert np.abs(desc - d_ref).max() <= 1e-6                            # float32 output of values <= 1
    # a capacity below the number found: the count is reported, nothing is written past the end, the head is the same
    kp2, rec2, resp2, found2 = _detect(emu, flat, h, w, o, max(n // 2, 1))
    assert found2 == n and np.array_equal(kp2, kp[:len(kp2)]) and np.array_equal(rec2, rec[:len(rec2)])


def test_bad_inputs_are_refused_and_leave_the_outputs_untouched(emu):
    lib, ctx = emu
    image = sc.textured_image(40, 37, 6)
    flat, _, o = _pyramid(emu, image)
    bad = [dict(first_octave=1), dict(first_octave=-2), dict(octave_resolution=1), dict(octave_resolution=5), dict(sigma0=1.0),
           dict(sigma0=0.5, first_octave=0), dict(num_octaves=-1), dict(num_octaves=5), dict(max_num_orientations=0),
           dict(max_num_orientations=5), dict(normalization=2), dict(edge_threshold=0.0)]
    for kw in bad:
        ob = _options(**kw)
        nbytes = C.c_int64(-9)
        assert lib.pxr_sift_pyramid_bytes(40, 37, C.byref(ob), C.byref(nbytes)) == -1 and nbytes.value == -9, kw
        out = np.full(flat.size, -7.0, np.float32)
        assert lib.pxr_sift_pyramid(ctx, _p(image), 3, 40, 37, C.byref(ob), _p(out)) == -1 and (out == -7).all(), kw
        with pytest.raises(ValueError, match="-1:"):
            _detect(emu, flat, 40, 37, ob, 8)
    for h, w in ((0, 37), (40, 0), (-1, 5)):
        with pytest.raises(ValueError, match="-1:.*size"):
            _detect(emu, flat, h, w, o, 8)
    found = C.c_int64(-9)
    assert lib.pxr_sift_detect(ctx, _p(flat), 40, 37, C.byref(o), C.c_int64(-1), None, None, None, C.byref(found)) == -1 and found.value == -9
    assert lib.pxr_sift_detect(ctx, _p(flat), 40, 37, C.byref(o), C.c_int64(4), None, None, None, C.byref(found)) == -1 and found.value == -9
    assert lib.pxr_sift_detect(ctx, None, 40, 37, C.byref(o), C.c_int64(0), None, None, None, C.byref(found)) == -1
    assert lib.pxr_sift_describe(ctx, _p(flat), 40, 37, C.byref(o), C.c_int64(-1), None, None, None) == -1
    assert lib.pxr_sift_describe(ctx, _p(flat), 40, 37, C.byref(o), C.c_int64(2), None, None, None) == -1
    assert lib.pxr_sift_pyramid(ctx, _p(image), 2, 40, 37, C.byref(o), _p(flat)) == -1           # PXR_F64 is no image dtype
    # capacity 0 counts without writing
    assert lib.pxr_sift_detect(ctx, _p(flat), 40, 37, C.byref(o), C.c_int64(0), None, None, None, C.byref(found)) == 0 and found.value > 0


def test_keypoints_that_cannot_be_described_get_zeros_and_leave_their_neighbours_alone(emu):
    image = sc.textured_image(40, 37, 6)
    flat, levels, o = _pyramid(emu, image)
    kp, _, _, found = _detect(emu, flat, 40, 37, o, 64)
    good = kp[:min(found, 6)]
    alone, valid_alone = _describe(emu, flat, 40, 37, o, good)
    assert valid_alone.all()
    nan, inf = np.nan, np.inf
    bad = np.array([[nan, 3, 2, 0], [3, inf, 2, 0], [3, 3, -1, 0], [3, 3, 0, 0], [3, 3, 2, nan], [3, 3, 1e-3, 0], [3, 3, 1e6, 0],
                    [1e300, -1e300, 2, 0], [-500, 20, 2, 0]])
    mixed = np.empty((len(good) + len(bad), 4))
    rows = [None] * len(mixed)
    gi = bi = 0
    for i in range(len(mixed)):                                                      # good and bad interleaved while both last
        if (i % 2 == 0 and gi < len(good)) or bi >= len(bad):
            rows[i] = ("g", gi); mixed[i] = good[gi]; gi += 1
        else:
            rows[i] = ("b", bi); mixed[i] = bad[bi]; bi += 1
    desc, valid = _describe(emu, flat, 40, 37, o, mixed)
    for i, (kind, j) in enumerate(rows):
        if kind == "g":
            assert valid[i] == 1 and np.array_equal(desc[i], alone[j])
        else:
            assert valid[i] == 0 and (desc[i] == 0).all(), bad[j]


def test_a_constant_image_has_no_features(emu):
    image = np.full((30, 41), 77, np.uint8)
    flat, levels, o = _pyramid(emu, image)
    assert all(np.abs(lv - np.float32(77) / np.float32(255)).max() < 1e-6 for lv in levels)
    assert _detect(emu, flat, 30, 41, o, 4)[3] == 0
    small = np.full((7, 9), 3, np.uint8)                                  # below 16 pixels even when doubled: no octave at all
    flat, levels, o = _pyramid(emu, small)
    assert levels == [] and _detect(emu, np.zeros(1, np.float32), 7, 9, o, 4)[3] == 0


def test_sanitized_stand_alone_program(tmp_path):
    """The same translation unit with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
    program whose arrays have their exact sizes: an image smaller than a tile, one with odd halving over two octaves and a
    capacity below the number found, and a capacity of zero."""
    for args, few in ((("17", "23", "-1", "64"), False), (("33", "37", "0", "3"), True), (("19", "21", "-1", "0"), True)):
        stdout = lanes.sanitized(tmp_path, "sift_on_host.cpp", "SIFT_ON_HOST_MAIN", *args)
        words = stdout.split()
        found, written, valid = int(words[1]), int(words[3]), int(words[5])
        assert found > 0 and written == min(found, int(args[3])) and valid == written, stdout
        assert (found > int(args[3])) == few, stdout
        assert words[7:] == ["0", "0", "0", "1", "0"], stdout          # only the large window in the middle can be described
