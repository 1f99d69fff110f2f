"""What the tests of batched map localization share: a second statement, in numpy and plain loops, of the three definitions in
include/pixsfm_hip.h (pxr_covisibility, pxr_covisibility_clusters, pxr_localization_pairs -- the clustering written as hloc
writes its breadth-first search), the boundary batch the kernels are held to bit for bit, every class of bad input, and a map of
two places with held-out queries for the end-to-end tests."""
import functools

import numpy as np

MAX_ENTRIES = 64          # PXR_MAX_LOC_ENTRIES


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def covisibility_reference(track_offsets, obs_image, n_images, track_mask=None):
    """count[i][j]: over the tracks that count, the ordered pairs (a, b) of observations with image(a) = i != j = image(b)."""
    off, img = np.asarray(track_offsets), np.asarray(obs_image)
    count = np.zeros((n_images, n_images), np.int32)
    for t in range(len(off) - 1):
        if track_mask is not None and not track_mask[t]:
            continue
        for a in range(off[t], off[t + 1]):
            for b in range(off[t], off[t + 1]):
                if img[a] != img[b]:
                    count[img[a], img[b]] += 1
    return count


def topk_reference(count, num_matched):
    """Per row the min(num_matched, positives) partners by (count descending, index ascending): (index, count, n), rows padded
    with -1 / 0."""
    n_images = len(count)
    index, cnt = np.full((n_images, num_matched), -1, np.int32), np.zeros((n_images, num_matched), np.int32)
    n = np.zeros(n_images, np.int32)
    for i in range(n_images):
        partners = sorted((j for j in range(n_images) if count[i, j] > 0), key=lambda j: (-count[i, j], j))[:num_matched]
        n[i] = len(partners)
        index[i, :n[i]] = partners
        cnt[i, :n[i]] = [count[i, j] for j in partners]
    return index, cnt, n


def clusters_of_list(count, ret):
    """hloc's do_covisibility_clustering over the ENTRIES of one retrieval list (an image listed twice is two entries, connected):
    the clusters as lists of entry positions, sorted by size (stable over discovery order)."""
    ret = [int(r) for r in ret]
    visited, clusters = set(), []
    for start in range(len(ret)):
        if start in visited:
            continue
        clusters.append([])
        queue = {start}
        while len(queue):
            e = queue.pop()
            if e in visited:
                continue
            visited.add(e)
            clusters[-1].append(e)
            connected = {f for f in range(len(ret)) if ret[f] == ret[e] or count[ret[e], ret[f]] > 0}     # only frames of the list
            connected -= visited
            queue |= connected
    # discovery order = order of the first member, since the outer loop walks the list in rank order
    clusters = sorted(clusters, key=len, reverse=True)
    return [sorted(c) for c in clusters]


def clusters_reference(count, ret_offsets, ret):
    """(cluster (n_ret,) int32, n_clusters (n_queries,) int32) of pxr_covisibility_clusters."""
    off, ret = np.asarray(ret_offsets), np.asarray(ret)
    cluster, n_clusters = np.full(len(ret), -1, np.int32), np.zeros(len(off) - 1, np.int32)
    for q in range(len(off) - 1):
        found = clusters_of_list(count, ret[off[q]:off[q + 1]])
        n_clusters[q] = len(found)
        for number, members in enumerate(found):
            for e in members:
                cluster[off[q] + e] = number
    return cluster, n_clusters


def pairs_reference(b):
    """The outputs of pxr_localization_pairs for a batch dict (see pairs_batch), the correspondence arrays cut to n_corr rows."""
    img_off, pair_off = b["image_offsets"], b["pair_offsets"]
    offsets, kp, point = [0], [], []
    for p in range(len(b["problem_offsets"]) - 1):
        entries = b["problem_pair"][b["problem_offsets"][p]:b["problem_offsets"][p + 1]]
        if len(entries):
            query = b["pairs"][entries[0], 0]
            for k in range(img_off[query + 1] - img_off[query]):
                if not np.isfinite(b["kp_xy"][img_off[query] + k]).all():
                    continue
                seen = []
                for pr in entries:
                    m = b["matches0"][pair_off[pr] + k]
                    if m < 0:
                        continue
                    pid = b["kp_point"][img_off[b["pairs"][pr, 1]] + m]
                    if pid < 0 or not np.isfinite(b["xyz"][pid]).all() or pid in seen:
                        continue
                    seen.append(int(pid))
                    kp.append((query, k))
                    point.append(int(pid))
        offsets.append(len(point))
    rows = np.array([img_off[q] + k for q, k in kp], np.int64)
    point = np.array(point, np.int64)
    return dict(corr_offsets=np.array(offsets, np.int64), n_corr=len(point), corr_kp=np.array([k for _, k in kp], np.int32),
                corr_point=point, corr_xy=b["kp_xy"][rows].reshape(-1, 2), corr_xyz=b["xyz"][point].reshape(-1, 3))


# ---- the boundary batch ----------------------------------------------------------------------------------------------------------
TRACK_LENGTHS = (1, 2, 15, 16, 17, 33, 300)       # around the 16 lanes a track gets, and many passes of them
COVIS_IMAGES = (1, 63, 64, 65)                    # around the wavefront
NUM_MATCHED = (1, 100)                            # one partner; more than any row has


def covis_batch(n_images, seed=3):
    """Tracks of TRACK_LENGTHS observations (the long one over at most 20 images: images see it many times), 40 short random
    tracks, a masked-out track of 40 observations that would change every count, an empty track; the last image observes
    nothing (n_images > 1).  Returns (track_offsets, obs_image, track_mask)."""
    rng = np.random.default_rng(seed + n_images)
    seeing = max(n_images - 1, 1)
    lengths = list(TRACK_LENGTHS) + [40, 0] + list(rng.integers(2, 7, 40))
    obs = [rng.integers(0, min(seeing, 20) if L == 300 else seeing, L) for L in lengths]
    mask = np.ones(len(lengths), np.uint8)
    mask[len(TRACK_LENGTHS)] = 0
    mask[0] = 5                                                       # any non-zero value counts
    order = rng.permutation(len(lengths))
    offsets = np.concatenate([[0], np.cumsum([lengths[t] for t in order])]).astype(np.int64)
    return offsets, np.concatenate([obs[t] for t in order]).astype(np.int32), mask[order]


def cluster_batch(seed=9):
    """A count matrix over 65 images made of chains: image i is covisible with i + 5 (five chains through the residues mod 5, a
    few links cut), so a component is only found by walking through several members, and chains of equal size compete for their
    number.  Lists of 0, 1, 63 (one image twice), 64 and 20 entries, the chain a-b-c, the same chain without b, and two
    clusters of equal size.  Returns (count, ret_offsets, ret)."""
    rng = np.random.default_rng(seed)
    n = 65
    count = np.zeros((n, n), np.int32)
    for i in range(n - 5):
        if i not in (12, 33, 41):
            count[i, i + 5] = count[i + 5, i] = rng.integers(1, 9)
    lists = [[], [17], list(rng.permutation(n)[:62]), list(rng.permutation(n)[:64]), list(rng.permutation(n)[:20]),
             [0, 10, 5], [0, 10], [6, 2, 7, 1]]
    lists[2].append(lists[2][3])                                      # 63 entries, one image twice
    lists[2] = [lists[2][k] for k in rng.permutation(63)]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return count, offsets, np.array([i for x in lists for i in x], np.int32)


def pairs_batch(seed=21):
    """Images 0 .. 3 are queries of 30, 0, 70 and 300 keypoints, images 4 .. 9 database images (one without keypoints); every
    (query, database) pair is matched at random.  Query 0 holds the hand-made keypoints: 3 reaches point 7 through three database
    images and point 9 through a fourth, 4 matches a keypoint without a point, 5 a point with NaN coordinates, 6 a point at
    infinity, and keypoint 8 itself is not finite.  Problems: all pairs of query 0 in shuffled order; none; two pairs; the
    query without keypoints; query 2; one pair of query 3; 64 entries (pairs repeat); query 3 in full; none.
    Returns the dict of the arguments of pxr_localization_pairs (host arrays)."""
    rng = np.random.default_rng(seed)
    n_kp = np.array([30, 0, 70, 300, 40, 25, 0, 33, 64, 90])
    n_q, n_set = 4, len(n_kp)
    img_off = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int64)
    n_points = 50
    xyz = rng.uniform(-2, 2, (n_points, 3))
    xyz[11, 1] = np.nan
    xyz[12, 2] = np.inf
    kp_xy = rng.uniform(0, 640, (img_off[-1], 2))
    kp_xy[img_off[0] + 8, 0] = np.nan
    kp_point = rng.integers(-1, n_points, img_off[-1]).astype(np.int64)
    kp_point[rng.uniform(size=len(kp_point)) < 0.3] = -1
    kp_point[kp_point == 12] = 13
    kp_point[kp_point == 11] = 13
    pairs = np.array([(q, d) for q in range(n_q) for d in range(n_q, n_set)], np.int32)
    pair_off = np.concatenate([[0], np.cumsum(n_kp[pairs[:, 0]])]).astype(np.int64)
    matches0 = np.full(pair_off[-1], -1, np.int32)
    for p, (q, d) in enumerate(pairs):
        if n_kp[d]:
            m = rng.integers(0, n_kp[d], n_kp[q])
            m[rng.uniform(size=n_kp[q]) < 0.4] = -1
            matches0[pair_off[p]:pair_off[p + 1]] = m

    def put(q, d, k, m, pid):                                         # query keypoint k of pair (q, d) -> database keypoint m, which sees pid
        matches0[pair_off[(q * (n_set - n_q)) + (d - n_q)] + k] = m
        kp_point[img_off[d] + m] = pid
    put(0, 4, 3, 1, 7); put(0, 5, 3, 2, 7); put(0, 7, 3, 0, 7); put(0, 8, 3, 1, 9); put(0, 9, 3, 4, -1)
    put(0, 4, 4, 5, -1); put(0, 5, 4, 6, -1); put(0, 7, 4, 6, -1); put(0, 8, 4, 7, -1); put(0, 9, 4, 7, -1)
    put(0, 4, 5, 6, 11)
    put(0, 4, 6, 7, 12)
    for d in (5, 7, 8, 9):                                            # keypoints 5 and 6 match nothing else
        matches0[pair_off[d - n_q] + 5] = matches0[pair_off[d - n_q] + 6] = -1
    per_q = n_set - n_q
    of = lambda q: list(range(q * per_q, (q + 1) * per_q))            # noqa: E731
    problems = [list(rng.permutation(of(0))), [], [of(0)[3], of(0)[0]], of(1)[:3], of(2), [of(3)[5]],
                list(rng.integers(0, per_q, 64)), of(3), []]
    problem_off = np.concatenate([[0], np.cumsum([len(x) for x in problems])]).astype(np.int64)
    return dict(problem_offsets=problem_off, problem_pair=np.array([e for x in problems for e in x], np.int32), pairs=pairs,
                pair_offsets=pair_off, matches0=matches0, image_offsets=img_off, kp_xy=kp_xy, kp_point=kp_point, xyz=xyz)


@functools.lru_cache(maxsize=None)
def boundary_batch():
    """One batch per entry point that holds every case its kernels can get wrong, with the reference outputs, computed once:
    dict(covis=[dict(n_images, track_offsets, obs_image, track_mask, count, topk={num_matched: (index, count, n)})],
    clusters=dict(count, ret_offsets, ret, cluster, n_clusters), pairs=dict(batch, ref)).  Treat it as read-only."""
    covis = []
    for n_images in COVIS_IMAGES:
        off, img, mask = covis_batch(n_images)
        count = covisibility_reference(off, img, n_images, mask)
        covis.append(dict(n_images=n_images, track_offsets=off, obs_image=img, track_mask=mask, count=count,
                          topk={k: topk_reference(count, k) for k in NUM_MATCHED}))
    count, ret_off, ret = cluster_batch()
    cluster, n_clusters = clusters_reference(count, ret_off, ret)
    batch = pairs_batch()
    return dict(covis=covis, clusters=dict(count=count, ret_offsets=ret_off, ret=ret, cluster=cluster, n_clusters=n_clusters),
                pairs=dict(batch=batch, ref=pairs_reference(batch)))


def _put(a, k, v):
    a = np.array(a)
    a[k] = v
    return a


def bad_covisibility(c):
    """(name, replaced arguments, a word of the message) for every class pxr_covisibility refuses; c: an entry of covis."""
    off, img, n = c["track_offsets"], c["obs_image"], c["n_images"]
    return [("offsets not starting at 0", dict(track_offsets=_put(off, 0, 1)), "not 0"),
            ("offsets not monotone", dict(track_offsets=_put(off, 3, off[4] + 1)), "monotone"),
            ("offsets not ending at n_obs", dict(track_offsets=_put(off, len(off) - 1, len(img) + 1)), "n_obs"),
            ("image index too large", dict(obs_image=_put(img, 5, n)), "image"),
            ("image index negative", dict(obs_image=_put(img, len(img) - 1, -1)), "image"),
            ("num_matched zero", dict(num_matched=0), "num_matched"),
            ("num_matched too large", dict(num_matched=257), "num_matched"),
            ("too many images", dict(n_images=8193), "PXR_MAX_COVIS_IMAGES")]


def bad_clusters(c):
    """The same for pxr_covisibility_clusters; c: the clusters entry."""
    off, ret = c["ret_offsets"], c["ret"]
    long_off = _put(off, slice(4, None), off[4:] + 1)                # the 64-entry list (query 3) takes one entry more
    return [("65 entries", dict(ret_offsets=long_off, ret=np.concatenate([ret, [0]]).astype(np.int32)), "more than 64"),
            ("offsets not starting at 0", dict(ret_offsets=_put(off, 0, 1)), "not 0"),
            ("offsets not monotone", dict(ret_offsets=_put(off, 5, off[6] + 1)), "monotone"),
            ("offsets not ending at n_ret", dict(ret_offsets=_put(off, len(off) - 1, len(ret) + 1)), "n_ret"),
            ("image index too large", dict(ret=_put(ret, 7, 65)), "image"),
            ("image index negative", dict(ret=_put(ret, 0, -1)), "image"),
            ("too many images", dict(n_images=8193), "PXR_MAX_COVIS_IMAGES")]


def bad_pairs(b):
    """The same for pxr_localization_pairs; b: the batch of pairs_batch."""
    po, pp, pairs, pair_off, img_off = b["problem_offsets"], b["problem_pair"], b["pairs"], b["pair_offsets"], b["image_offsets"]
    long_off = _put(po, slice(7, None), po[7:] + 1)                  # the 64-entry problem (6) takes one entry more
    two_queries = _put(pp, po[4] + 1, 0)                             # a pair of query 0 among those of query 2
    first_match = int(np.flatnonzero(b["matches0"] >= 0)[0])
    return [("65 entries", dict(problem_offsets=long_off, problem_pair=np.concatenate([pp[:po[7]], [0], pp[po[7]:]]).astype(np.int32)), "more than 64"),
            ("two queries in one problem", dict(problem_pair=two_queries), "share"),
            ("problem offsets not starting at 0", dict(problem_offsets=_put(po, 0, 1)), "not 0"),
            ("problem offsets not monotone", dict(problem_offsets=_put(po, 1, po[2] + 1)), "monotone"),
            ("problem offsets not ending at n_entries", dict(problem_offsets=_put(po, len(po) - 1, len(pp) + 1)), "n_entries"),
            ("pair offsets not starting at 0", dict(pair_offsets=_put(pair_off, 0, 1)), "not 0"),
            ("pair rows differ from the keypoint count", dict(pair_offsets=_put(pair_off, 1, pair_off[1] - 1)), "rows"),
            ("image offsets not monotone", dict(image_offsets=_put(img_off, 3, img_off[4] + 1)), "monotone"),
            ("image offsets not ending at n_total", dict(image_offsets=_put(img_off, len(img_off) - 1, img_off[-1] - 1)), "n_total"),
            ("entry out of range", dict(problem_pair=_put(pp, 2, len(pairs))), "pair"),
            ("entry negative", dict(problem_pair=_put(pp, 2, -1)), "pair"),
            ("image of a pair out of range", dict(pairs=_put(pairs, (5, 1), len(img_off) - 1)), "image"),
            ("match beyond the database keypoints", dict(matches0=_put(b["matches0"], first_match, 1000)), "keypoint"),
            ("point out of range", dict(kp_point=_put(b["kp_point"], slice(None), np.where(b["kp_point"] == 7, len(b["xyz"]), b["kp_point"]))),
             "point")]


# ---- a map of two places -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_places(n_queries=4, seed=4):
    """mapping_cases.ring_scene with a second ring far away (8 + 6 images), exact keypoints with unit-norm random descriptors per
    point (so that nearest neighbours are the true matches); images 0, 1 of the first ring and 8, 9 of the second are held out as
    queries and the map is the ground-truth reconstruction of the rest.  Returns dict(scene, reconstruction, queries,
    place {name: 0 / 1}, descriptors {name: (n, 32) float32}, retrieval {query: db names, both places interleaved})."""
    import mapping_cases as mc
    from pixsfm_amd.api.reconstruction import Image, Point2D, Point3D, Reconstruction, Track, TrackElement
    scene = mc.ring_scene(n_images=8, n_points=120, views=5, sigma=0.3, seed=seed, n_images_second=6)
    rng = np.random.default_rng(seed)
    desc_of_point = rng.normal(size=(len(scene["X"]), 32)).astype(np.float32)
    desc_of_point /= np.linalg.norm(desc_of_point, axis=1, keepdims=True)
    names = scene["names"]
    place = {nm: int(i >= 8) for i, nm in enumerate(names)}
    queries = [names[0], names[1], names[8], names[9]][:n_queries]
    db = [nm for nm in names if nm not in queries]
    descriptors = {nm: desc_of_point[scene["owner"][nm]] for nm in names}
    rec = Reconstruction()
    rec.add_camera(scene["camera"])
    seen = {}
    for image_id, nm in enumerate(db, 1):
        q, t = scene["poses"][nm]
        rec.add_image(Image(image_id, nm, 1, q, t, [Point2D(xy, int(pid)) for xy, pid in zip(scene["keypoints"][nm], scene["owner"][nm])]))
        for k, pid in enumerate(scene["owner"][nm]):
            seen.setdefault(int(pid), []).append(TrackElement(image_id, k))
    for pid, elements in seen.items():
        rec.add_point3D(pid, Point3D(scene["X"][pid], Track(elements)))
    by_place = [[nm for nm in db if place[nm] == s] for s in (0, 1)]
    retrieval = {}
    for qn in queries:
        mine, other = by_place[place[qn]], by_place[1 - place[qn]]
        mixed = [nm for pair in zip(other, mine) for nm in pair] + mine[len(other):] + other[len(mine):]
        retrieval[qn] = mixed
    return dict(scene=scene, reconstruction=rec, queries=queries, place=place, descriptors=descriptors, retrieval=retrieval)
