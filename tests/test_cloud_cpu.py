"""The brute-force statement of the cloud evaluation (tests/cloud_cases.py) against an independent implementation and against
its own defining properties -- what the lane-emulation and GPU tests then hold the kernels to bit for bit."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import cloud_cases as cc


@pytest.mark.parametrize("seed,n_ref,n_query,max_dist", [(0, 500, 400, 0.2), (1, 3000, 1000, 0.05), (2, 64, 257, 1.0), (3, 1, 50, 1.5)])
def test_brute_force_agrees_with_a_kd_tree(seed, n_ref, n_query, max_dist):
    rng = np.random.default_rng(seed)
    ref, query = rng.uniform(-1, 1, (n_ref, 3)), rng.uniform(-1, 1, (n_query, 3))
    index, dist2 = cc.nearest(ref, query, max_dist)
    d, j = cKDTree(ref).query(query, k=2 if n_ref > 1 else 1, distance_upper_bound=max_dist)
    d, j = d.reshape(n_query, -1), j.reshape(n_query, -1)
    found = np.isfinite(d[:, 0])
    # cKDTree sums the squares in another order: 4 ulps of the coordinates' magnitude (|x| <= 1) on the distances
    tol = 4 * np.spacing(1.0)
    boundary = np.abs(np.where(found, d[:, 0], max_dist) - max_dist) <= tol                # (a pair that close to max_dist may go either way)
    boundary |= np.abs(np.sqrt(np.where(index >= 0, dist2, max_dist ** 2)) - max_dist) <= tol
    assert np.array_equal((index >= 0) | boundary, found | boundary)
    both = found & (index >= 0)
    assert both.sum() > 0
    assert np.abs(np.sqrt(dist2[both]) - d[both, 0]).max() <= tol
    with np.errstate(invalid="ignore"):                                                    # (inf - inf where nothing was found)
        unique = both & (d[:, -1] - d[:, 0] > tol) if d.shape[1] > 1 else both             # the nearest is unique
    assert np.array_equal(index[unique], j[unique, 0])
    assert (index[~found & ~boundary] == -1).all() and np.isposinf(dist2[index < 0]).all()


def test_a_query_that_is_a_reference_point_finds_itself():
    ref, query, max_dist = cc.NEAREST_CASES["duplicates"]
    index, dist2 = cc.nearest_reference("duplicates")
    n_self = len(ref[::3])
    assert (dist2[:n_self] == 0).all()
    own = np.arange(0, len(ref), 3)
    assert (index[:n_self] <= own).all()                              # itself, or the lower-indexed duplicate
    assert np.array_equal(ref[index[:n_self]], ref[own])
    assert (index[:n_self] < own).any()
    ref, _, _ = cc.NEAREST_CASES["identical"]
    index, dist2 = cc.nearest_reference("identical")
    assert np.array_equal(index, np.arange(len(ref))) and (dist2 == 0).all()


def test_pairs_at_exactly_max_dist_are_candidates_and_one_ulp_outside_are_not():
    for s in cc.EXACT_SCALES:
        for name, (ref, query, max_dist, inside) in cc.exact_pairs(s).items():
            index, dist2 = cc.nearest(ref, query, max_dist)
            # (the queries repeat: the references at +offset and -offset around one query tie, the lowest index wins)
            own = np.flatnonzero(inside)
            assert (index[inside] >= 0).all() and (index[inside] <= own).all() and (index[inside] < own).any(), name
            assert (dist2[inside] == max_dist * max_dist).all(), name
            assert (index[~inside] == -1).all() and np.isposinf(dist2[~inside]).all(), name


def test_rows_that_are_not_finite_never_match():
    ref, query, _ = cc.NEAREST_CASES["not_finite"]
    index, dist2 = cc.nearest_reference("not_finite")
    assert (index[~cc.valid_rows(query)] == -1).all()
    assert cc.valid_rows(ref)[index[index >= 0]].all()
    assert index[10] == 6 and dist2[10] == 0


def test_voxel_fractions_with_size_zero_are_the_plain_ratio():
    xyz, dist2, v, tol = cc.VOXEL_CASES["zero_size"]
    frac, n_vox = cc.voxel_reference("zero_size")
    assert n_vox == len(xyz)
    for k, t in enumerate(tol):
        assert frac[k] == float((dist2 <= t * t).sum()) / float(len(xyz))


@pytest.mark.parametrize("name", ["faces", "random_5000", "eight_tolerances", "not_finite", "zero_size"])
def test_voxel_fractions_do_not_depend_on_the_order_of_the_points(name):
    xyz, dist2, v, tol = cc.VOXEL_CASES[name]
    frac, n_vox = cc.voxel_reference(name)
    perm = np.random.default_rng(1).permutation(len(xyz))
    frac_p, n_vox_p = cc.voxel_fractions(xyz[perm], dist2[perm], v, tol)
    assert n_vox_p == n_vox and frac_p.tobytes() == frac.tobytes()


def test_voxel_floor_is_not_a_truncation():
    xyz = np.array([[-0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [-0.9, 0.9, 0.9], [-1.0, 0.0, 0.0], [-1.0 - 1e-9, 0.0, 0.0]])
    frac, n_vox = cc.voxel_fractions(xyz, np.array([0.0, 1.0, 1.0, 0.0, 1.0]), 1.0, [0.5])
    assert n_vox == 3                                                  # {0, 2, 3} in (-1, 0, 0), {1} in (0, 0, 0), {4} in (-2, 0, 0)
    q = int(np.rint((2.0 / 3.0) * 2.0 ** 32))                          # the fixed-point share of the first voxel; the others are 0
    assert q == 2863311531 and frac[0] == float(q) * 2.0 ** -32 / 3.0


def test_voxel_range_and_empty_input():
    assert cc.voxel_reference("out_of_range") is None and cc.voxel_reference("out_of_range_negative") is None
    assert cc.voxel_reference("range_edge") is not None
    for name in ("no_valid_point", "empty"):
        frac, n_vox = cc.voxel_reference(name)
        assert n_vox == 0 and np.isnan(frac).all()
    frac, _ = cc.voxel_reference("all_within")
    assert (frac == 1.0).all()
