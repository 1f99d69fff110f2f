"""The host-side structure of a BA solve (csrc/pxr_ba_structure.h: block layout, observation lists, chunkings, preconditioner
blocks, column-entry tables) without a GPU: tests/host/ba_structure_main.cpp is built with AddressSanitizer and UBSan and run as a
program on tiny problems; its tables are held to a restatement of the rules in numpy, to one table written out by hand, and to
the invariants the kernels rely on."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]        # COLMAP camera models by id
SIMPLE_PINHOLE, PINHOLE, OPENCV, FULL_OPENCV = 0, 1, 4, 6
GS = 18                                                  # PCG_GS: rows of the largest preconditioner block


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no g++"
    out = str(tmp_path_factory.mktemp("structure") / "ba_structure_main")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "pixel-perfect-sfm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "ba_structure_main.cpp"), "-o", out])
    return out


def _case(image_camera, cam_model, pose_const, tvec_mask, cam_mask, point_const, obs_image, obs_point):
    return dict(image_camera=np.asarray(image_camera, np.int64), cam_model=np.asarray(cam_model, np.int64),
                pose_const=np.asarray(pose_const, np.int64), tvec_mask=np.asarray(tvec_mask, np.int64),
                cam_mask=np.asarray(cam_mask, np.int64), point_const=np.asarray(point_const, np.int64),
                obs_image=np.asarray(obs_image, np.int64), obs_point=np.asarray(obs_point, np.int64))


def _run(program, c):
    keys = ("image_camera", "cam_model", "pose_const", "tvec_mask", "cam_mask", "point_const", "obs_image", "obs_point")
    dims = [len(c["image_camera"]), len(c["cam_model"]), len(c["point_const"]), len(c["obs_image"])]
    text = " ".join(str(int(v)) for v in dims + [x for k in keys for x in c[k]])
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=20)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]          # a sanitizer report ends the program with a message
    return json.loads(r.stdout)


# ---- the rules, restated -----------------------------------------------------------------------------------------------------------
def _popcount(x):
    return bin(int(x)).count("1")


def _expected(c):
    n_img, n_cam, n_pts, n_obs = len(c["image_camera"]), len(c["cam_model"]), len(c["point_const"]), len(c["obs_image"])
    e = {}
    e["tmask"] = [int(m) & 7 for m in c["tvec_mask"]]
    e["pose_dim"] = [0 if c["pose_const"][i] else 6 - _popcount(e["tmask"][i]) for i in range(n_img)]
    e["cmask"] = [int(c["cam_mask"][k]) & ((1 << NUM_PARAMS[c["cam_model"][k]]) - 1) for k in range(n_cam)]
    e["intr_dim"] = [NUM_PARAMS[c["cam_model"][k]] - _popcount(e["cmask"][k]) for k in range(n_cam)]
    offs = np.concatenate([[0], np.cumsum(e["pose_dim"] + e["intr_dim"])])          # pose blocks first, then intrinsics blocks
    e["pose_off"], e["intr_off"] = offs[:n_img].tolist(), offs[n_img:n_img + n_cam].tolist()
    e["n_c"] = int(offs[-1])
    e["DC"] = max(1, max(e["pose_dim"], default=0) + max(e["intr_dim"], default=0))
    e["LS"] = 11 + 2 * e["DC"]
    # observation lists: counting sort by image / by point, ascending observation id inside a bucket
    e["img_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(c["obs_image"], minlength=n_img))]).tolist()
    e["pt_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(c["obs_point"], minlength=n_pts))]).tolist()
    e["img_obs"] = np.argsort(c["obs_image"], kind="stable").tolist()
    e["pt_obs"] = np.argsort(c["obs_point"], kind="stable").tolist()
    e["pt_var"] = [int(not c["point_const"][p] and e["pt_ptr"][p + 1] > e["pt_ptr"][p]) for p in range(n_pts)]
    e["n_pvar"] = sum(e["pt_var"])
    for per in (512, 1024):
        chunks = [[i, b, min(e["img_ptr"][i + 1], b + per)] for i in range(n_img) for b in range(e["img_ptr"][i], e["img_ptr"][i + 1], per)]
        e["chunks%d" % per] = chunks
        e["first%d" % per] = np.concatenate([[0], np.cumsum(np.bincount([ch[0] for ch in chunks], minlength=n_img))]).astype(int).tolist()
    # preconditioner blocks: per image its pose columns, joined by the intrinsics of a camera only this image uses; then the shared cameras
    users = np.bincount(c["image_camera"], minlength=n_cam)
    groups = []
    for i in range(n_img):
        k = int(c["image_camera"][i])
        cols = list(range(e["pose_off"][i], e["pose_off"][i] + e["pose_dim"][i]))
        joint = users[k] == 1 and e["intr_dim"][k] > 0
        if joint:
            cols += list(range(e["intr_off"][k], e["intr_off"][k] + e["intr_dim"][k]))
        if e["pose_dim"][i] > 0 or joint:
            groups.append(cols)
    groups += [list(range(e["intr_off"][k], e["intr_off"][k] + e["intr_dim"][k])) for k in range(n_cam) if users[k] != 1 and e["intr_dim"][k] > 0]
    e["group_size"] = [len(g) for g in groups]
    e["group_cols"] = [x for g in groups for x in g + [0] * (GS - len(g))]
    e["col_group"] = [None] * e["n_c"]
    for gi, g in enumerate(groups):
        for r, col in enumerate(g):
            e["col_group"][col] = [gi, r]
    # column entries: (image, local column) of every global column, images ascending
    def column(i, a):
        k = c["image_camera"][i]
        return e["pose_off"][i] + a if a < e["pose_dim"][i] else e["intr_off"][k] + (a - e["pose_dim"][i])
    ent = sorted((column(i, a), i, a) for i in range(n_img) for a in range(e["pose_dim"][i] + e["intr_dim"][c["image_camera"][i]]))
    e["ent"] = [[i, a] for _, i, a in ent]
    e["ent_ptr"] = np.concatenate([[0], np.cumsum(np.bincount([col for col, _, _ in ent], minlength=e["n_c"]))]).astype(int).tolist()
    return e


def _check_invariants(c, got):
    n_img, n_obs, n_c = len(c["image_camera"]), len(c["obs_image"]), got["n_c"]
    # every column in exactly one preconditioner block, at the row the block lists it
    seen = np.zeros(n_c, int)
    for g, size in enumerate(got["group_size"]):
        assert 0 < size <= GS
        for r in range(size):
            col = got["group_cols"][g * GS + r]
            seen[col] += 1
            assert got["col_group"][col] == [g, r]
    assert (seen == 1).all()
    # the entries of a column: ascending images, as many as the column has users
    users = np.zeros(n_c, int)
    for i in range(n_img):
        k = c["image_camera"][i]
        users[got["pose_off"][i]:got["pose_off"][i] + got["pose_dim"][i]] += 1
        users[got["intr_off"][k]:got["intr_off"][k] + got["intr_dim"][k]] += 1
    for col in range(n_c):
        rows = got["ent"][got["ent_ptr"][col]:got["ent_ptr"][col + 1]]
        assert len(rows) == users[col] and [r[0] for r in rows] == sorted(set(r[0] for r in rows))
    assert got["ent_ptr"][n_c] == len(got["ent"])
    # the chunks tile every image's slots exactly
    for per in (512, 1024):
        chunks, first = got["chunks%d" % per], got["first%d" % per]
        for i in range(n_img):
            mine = chunks[first[i]:first[i + 1]]
            assert all(ch[0] == i and 0 < ch[2] - ch[1] <= per for ch in mine)
            edges = [got["img_ptr"][i]] + [ch[2] for ch in mine]
            assert [ch[1] for ch in mine] == edges[:-1] and edges[-1] == got["img_ptr"][i + 1]
        assert first[n_img] == len(chunks)
    # stable permutations
    for lst, ptr, key in ((got["img_obs"], got["img_ptr"], c["obs_image"]), (got["pt_obs"], got["pt_ptr"], c["obs_point"])):
        assert sorted(lst) == list(range(n_obs))
        for b in range(len(ptr) - 1):
            ids = lst[ptr[b]:ptr[b + 1]]
            assert ids == sorted(ids) and all(key[o] == b for o in ids)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _case_a():
    """3 images, 2 cameras: camera 0 (SIMPLE_PINHOLE) shared by images 0 and 1, camera 1 (OPENCV) used by image 2 alone -- a joint
    block.  Image 0 pose-constant, image 1 with t_y constant, one intrinsic of camera 1 masked."""
    return _case([0, 0, 1], [SIMPLE_PINHOLE, OPENCV], [1, 0, 0], [0, 0b010, 0], [0, 0b100], [0, 0, 0, 0],
                 [0, 1, 2, 1, 2, 0, 2, 0, 1], [0, 0, 0, 1, 1, 2, 2, 3, 3])


def _case_b():
    """camera 0 fully constant (intr_dim 0: its image's block holds the pose alone); image 1 pose-constant with a single-user
    camera (a block of the intrinsics alone); (tvec mask bits above 3 and mask bits beyond the model's parameters are ignored)"""
    return _case([0, 1], [OPENCV, SIMPLE_PINHOLE], [0, 1], [0b1000, 0b111], [0xffff, 0b1000], [0, 0, 0],
                 [0, 1, 0, 1, 0, 1], [0, 0, 1, 1, 2, 2])


def _case_c():
    """image 1 without an observation, point 2 without an observation, point 1 constant"""
    return _case([0, 0, 1, 1], [SIMPLE_PINHOLE, OPENCV], [1, 0, 0, 0], [0, 0, 0b001, 0], [0b010, 0], [0, 1, 0, 0],
                 [0, 2, 3, 0, 2, 0, 3], [0, 0, 0, 1, 1, 3, 3])


def _case_d():
    """case (a) with the observations in an order that is not by point"""
    c = _case_a()
    perm = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    return dict(c, obs_image=c["obs_image"][perm], obs_point=c["obs_point"][perm])


def _case_e():
    """image 0 with 1025 observations, image 1 with 513: both chunk sizes cross a boundary"""
    pts = np.arange(1025)
    obs_point = np.sort(np.concatenate([pts, pts[:513]]), kind="stable")
    obs_image = np.where(np.concatenate([[False], obs_point[1:] == obs_point[:-1]]), 1, 0)
    return _case([0, 1], [SIMPLE_PINHOLE, SIMPLE_PINHOLE], [1, 0], [0, 0], [0b110, 0b110], np.zeros(1025, int), obs_image, obs_point)


def _case_f():
    """the widest layout: two images with a FULL_OPENCV camera each, nothing constant -- two joint blocks that fill all GS rows"""
    return _case([0, 1], [FULL_OPENCV, FULL_OPENCV], [0, 0], [0, 0], [0, 0], [0, 0, 0], [0, 1, 0, 1, 0, 1], [0, 0, 1, 1, 2, 2])


def _case_g():
    """case (f) with ONE FULL_OPENCV camera shared by both images: two pose blocks and a block of the 12 intrinsics"""
    return dict(_case_f(), image_camera=np.asarray([0, 0], np.int64), cam_model=np.asarray([FULL_OPENCV], np.int64),
                cam_mask=np.asarray([0], np.int64))


def _case_h():
    """the mixture of tests/test_ba_wide_blocks_gpu.py's scene k: 8 images with a camera each, FULL_OPENCV (all refined) and PINHOLE
    (principal point constant); images 0 and 2 pose-constant, t_x of image 1 and t_x, t_z of image 3 constant, every seventh point
    constant; tracks of 4"""
    models = [FULL_OPENCV] + [FULL_OPENCV, PINHOLE] * 3 + [FULL_OPENCV]
    n_pts = 15
    obs_point = np.repeat(np.arange(n_pts), 4)
    obs_image = np.concatenate([(p + 3 * np.arange(4)) % 8 for p in range(n_pts)])
    return _case(list(range(8)), models, [1, 0, 1, 0, 0, 0, 0, 0], [0, 1, 0, 0b101, 0, 0, 0, 0],
                 [0b1100 if m == PINHOLE else 0 for m in models], [int(p % 7 == 0) for p in range(n_pts)], obs_image, obs_point)


CASES = {"a": _case_a, "b": _case_b, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f, "g": _case_g, "h": _case_h}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_match_the_restated_rules(program, name):
    c = CASES[name]()
    got, want = _run(program, c), _expected(c)
    assert "error" not in got
    for key, value in want.items():
        assert got[key] == value, key
    assert set(got) == set(want)
    _check_invariants(c, got)


def test_smallest_case_by_hand(program):
    """Case (a), written out: columns 0-4 pose of image 1 (t_y constant), 5-10 pose of image 2, 11-13 camera 0, 14-20 camera 1."""
    got = _run(program, _case_a())
    assert (got["pose_off"], got["pose_dim"], got["tmask"]) == ([0, 0, 5], [0, 5, 6], [0, 2, 0])
    assert (got["intr_off"], got["intr_dim"], got["cmask"]) == ([11, 14], [3, 7], [0, 4])
    assert (got["n_c"], got["DC"], got["LS"]) == (21, 13, 37)
    assert got["img_ptr"] == [0, 3, 6, 9] and got["img_obs"] == [0, 5, 7, 1, 3, 8, 2, 4, 6]
    assert got["pt_ptr"] == [0, 3, 5, 7, 9] and got["pt_obs"] == list(range(9)) and got["pt_var"] == [1, 1, 1, 1] and got["n_pvar"] == 4
    assert got["chunks512"] == got["chunks1024"] == [[0, 0, 3], [1, 3, 6], [2, 6, 9]] and got["first512"] == [0, 1, 2, 3]
    # blocks: pose of image 1; pose of image 2 joined by camera 1 (its only user); camera 0 (two users) on its own
    assert got["group_size"] == [5, 13, 3]
    assert got["col_group"] == [[0, r] for r in range(5)] + [[1, r] for r in range(6)] + [[2, r] for r in range(3)] + [[1, r] for r in range(6, 13)]
    assert got["group_cols"][:5] == [0, 1, 2, 3, 4] and got["group_cols"][GS:GS + 13] == [5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18, 19, 20]
    assert got["group_cols"][2 * GS:2 * GS + 3] == [11, 12, 13] and len(got["group_cols"]) == 3 * GS
    # camera 0's columns are local columns 0-2 of image 0 (no pose columns) and 5-7 of image 1
    assert got["ent_ptr"] == list(range(12)) + [13, 15, 17] + list(range(18, 25))
    assert got["ent"] == [[1, a] for a in range(5)] + [[2, a] for a in range(6)] + [[0, 0], [1, 5], [0, 1], [1, 6], [0, 2], [1, 7]] + \
        [[2, a] for a in range(6, 13)]


def test_widest_layout_by_hand(program):
    """FULL_OPENCV with everything refined: DC = 18 = GS.  A camera per image: two joint blocks of 18 rows, no padding column; one
    camera for both images: blocks of 6, 6 and 12 rows, every intrinsics column with an entry from each image."""
    got = _run(program, _case_f())
    assert (got["n_c"], got["DC"], got["LS"]) == (36, 18, 47)
    assert got["pose_off"] == [0, 6] and got["intr_off"] == [12, 24] and got["intr_dim"] == [12, 12]
    assert got["group_size"] == [GS, GS] and len(got["group_cols"]) == 2 * GS
    assert got["group_cols"] == list(range(0, 6)) + list(range(12, 24)) + list(range(6, 12)) + list(range(24, 36))
    assert got["ent_ptr"] == list(range(37))
    got = _run(program, _case_g())
    assert (got["n_c"], got["DC"], got["LS"]) == (24, 18, 47)
    assert got["group_size"] == [6, 6, 12]
    assert got["group_cols"][2 * GS:2 * GS + 12] == list(range(12, 24)) and len(got["group_cols"]) == 3 * GS
    assert got["ent_ptr"] == list(range(13)) + list(range(14, 37, 2))
    assert got["ent"][12:] == [[i, 6 + a] for a in range(12) for i in (0, 1)]


def test_mixed_widths_by_hand(program):
    """Case (h): blocks of 12 / 17 / 2 / 16 / 8 / 18 / 8 / 18 columns per image under DC = 18."""
    c = _case_h()
    got = _run(program, c)
    assert got["pose_dim"] == [0, 5, 0, 4, 6, 6, 6, 6] and got["intr_dim"] == [12, 12, 2, 12, 2, 12, 2, 12]
    assert (got["n_c"], got["DC"], got["LS"]) == (33 + 66, 18, 47)
    assert got["group_size"] == [12, 17, 2, 16, 8, 18, 8, 18]              # every camera has one user: joint blocks throughout
    assert got["pt_var"] == [int(p % 7 != 0) for p in range(15)] and got["n_pvar"] == 12
    assert np.bincount(c["obs_image"], minlength=8).min() > 0


def test_chunk_boundaries(program):
    got = _run(program, _case_e())
    assert got["img_ptr"] == [0, 1025, 1538]
    assert got["chunks512"] == [[0, 0, 512], [0, 512, 1024], [0, 1024, 1025], [1, 1025, 1537], [1, 1537, 1538]] and got["first512"] == [0, 3, 5]
    assert got["chunks1024"] == [[0, 0, 1024], [0, 1024, 1025], [1, 1025, 1538]] and got["first1024"] == [0, 2, 3]


def test_every_block_constant_is_an_error(program):
    c = _case([0, 0], [SIMPLE_PINHOLE], [1, 1], [0, 0], [0b111], [1, 0], [0, 1], [0, 0])          # point 1: variable, but no observation
    assert _run(program, c)["error"] == "pxr_ba_solve: every parameter block is constant"


@pytest.mark.parametrize("obs_image,obs_point,word", [([0, 3], [0, 1], "observation 1 references image 3 / point 1 out of range"),
                                                      ([0, 1], [-1, 1], "observation 0 references image 0 / point -1 out of range"),
                                                      ([0, 1], [0, 2], "observation 1 references image 1 / point 2 out of range")])
def test_out_of_range_indices_are_an_error(program, obs_image, obs_point, word):
    c = _case([0, 0, 0], [SIMPLE_PINHOLE], [0, 0, 0], [0, 0, 0], [0], [0, 0], obs_image, obs_point)
    assert _run(program, c)["error"] == "pxr_ba_solve: " + word


def test_unsupported_camera_model_is_an_error(program):
    c = _case([0], [11], [0], [0], [0], [0], [0], [0])
    assert _run(program, c)["error"] == "pxr_ba_solve: unsupported camera model id 11"
