"""Path-directed inputs for the binning of a scan (scan_keys_kernel -> bin_offsets_kernel -> bin_place_kernel, kernels.hip): queries
that fall into buckets of KNOWN sizes around the two cuts bin_offsets_kernel makes -- a bucket is cut every 64 queries, a last piece
of <= 16 queries is a LIGHT chunk (second list, growing down from the top of the chunk buffer), a longer one a normal chunk -- and a
map of more than 2046 occupied cubes, where the grouping key falls back from half-cell octants to whole cells.  Plain numpy: the
grouping key restated, the scan builder, the chunk counts that follow from a bucket-size histogram.  test_sampling_edges_host.py
asserts the properties on the CPU; test_gpu_sampling_edges.py runs the scans."""
import numpy as np

import knn_edge_data as ked

SIZES = (1, 16, 17, 63, 64, 65, 80, 81, 128, 129)  # around the light limit (16 / 17), the cut (63 / 64 / 65), both together (80 / 81), two cuts
LIGHT_MAX = 16
CLUSTER_HALF = 0.03   # queries of one bucket: within this of the anchor on every axis
FACE_MARGIN = 0.08    # the anchor: at least this far inside its half-cell octant on every axis


def half_cell(points, plane_res):
    """int64 [n, 3]: the half-cell (index inside the cube, 0 .. 2 nc - 1) of every point -- its low bit is the octant of the map cell"""
    nc, cell = ked.grid_cells(plane_res)
    u = (np.asarray(points, np.float32).astype(np.float64) + 25.0) % ked.CUBE / (cell / 2)
    return np.minimum(np.floor(u).astype(np.int64), 2 * nc - 1)


def grouping_key(points, plane_res):
    """int64 [n, 6]: cube, then half-cell octant -- the key scan_keys_kernel groups the kept queries of a located cube by (its 21-bit form)"""
    return np.concatenate([ked.cube_of(points), half_cell(points, plane_res)], axis=1)


def bucket_sizes(points, plane_res):
    """sizes of the buckets the queries fall into (one per distinct key), ascending"""
    _, cnt = np.unique(grouping_key(points, plane_res), axis=0, return_counts=True)
    return np.sort(cnt)


def chunks_of(count):
    """(normal chunks, light chunks) bin_offsets_kernel cuts a bucket of `count` queries into"""
    full, r = divmod(int(count), 64)
    return full + (1 if r > LIGHT_MAX else 0), 1 if 0 < r <= LIGHT_MAX else 0


def chunk_totals(sizes):
    pairs = [chunks_of(c) for c in sizes]
    return sum(p[0] for p in pairs), sum(p[1] for p in pairs)


def bucket_scan(map_points, plane_res, per_size=30, seed=17):
    """A scan (world frame: registered under the identity pose) whose queries fall into per_size buckets of every size of SIZES.
    A bucket is a cluster of +-CLUSTER_HALF around a map point that sits FACE_MARGIN inside its half-cell octant: on a surface of the
    scene, inside one cube that holds map points, inside one octant whatever the rounding of the key's arithmetic.  Buckets in
    shuffled order, their queries shuffled through the whole scan.  Returns (scan float32 [n, 3], bucket number of every query)."""
    rng = np.random.default_rng(seed)
    mp = np.asarray(map_points, np.float32)
    nc, cell = ked.grid_cells(plane_res)
    u = (mp.astype(np.float64) + 25.0) % ked.CUBE / (cell / 2)
    inside = ((u - np.floor(u) >= FACE_MARGIN / (cell / 2)) & (u - np.floor(u) <= 1.0 - FACE_MARGIN / (cell / 2))).all(1)
    # (a cluster stays inside the anchor's cube as well: cube faces are octant faces)
    cand = np.nonzero(inside)[0]
    _, first = np.unique(grouping_key(mp[cand], plane_res), axis=0, return_index=True)
    anchors = cand[rng.permutation(np.sort(first))]
    sizes = np.repeat(np.array(SIZES), per_size)
    assert len(anchors) >= len(sizes), (len(anchors), len(sizes))
    sizes = sizes[rng.permutation(len(sizes))]
    pts, owner = [], []
    for b, (a, s) in enumerate(zip(anchors, sizes)):
        pts.append(mp[a].astype(np.float64) + rng.uniform(-CLUSTER_HALF, CLUSTER_HALF, (s, 3)))
        owner.append(np.full(s, b))
    pts, owner = np.concatenate(pts), np.concatenate(owner)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(np.float32)), owner[order]


# ------------------------------------------------------------------------------------------------------------------------
# more than 2046 occupied cubes: the whole-cell key (cell_bits == 18)
# ------------------------------------------------------------------------------------------------------------------------
WINDOW = (21, 21, 11)          # cubes of the map window (local_map.h), centred on cube 0 for a sensor near the origin
KEY_SLOT_LIMIT = 2046          # occupied cubes the 21-bit key has room for (scan_keys_kernel: n_slots + 2 <= 2048)


def far_cube_points(n_cubes=2100, seed=23):
    """five points near the centre of each of n_cubes cubes of the window that lie outside the 5 x 5 x 3 block of cubes around cube 0
    (not counted into the registration's map size, 90 m or more from any query within 35 m of the origin).  Returns (points, cubes)."""
    rng = np.random.default_rng(seed)
    hx, hy, hz = (w // 2 for w in WINDOW)
    g = np.stack(np.meshgrid(np.arange(-hx, hx + 1), np.arange(-hy, hy + 1), np.arange(-hz, hz + 1), indexing="ij"), -1).reshape(-1, 3)
    g = g[(np.abs(g[:, 0]) > 2) | (np.abs(g[:, 1]) > 2) | (np.abs(g[:, 2]) > 1)]
    g = g[rng.permutation(len(g))[:n_cubes]]
    assert len(g) == n_cubes
    off = np.array([[0, 0, 0], [2.3, 0, 0], [0, 2.3, 0], [0, 0, 2.3], [2.3, 2.3, 0]], float)  # (apart by more than any planeRes leaf in use)
    return np.ascontiguousarray((g[:, None, :] * ked.CUBE + off[None, :, :]).reshape(-1, 3).astype(np.float32)), g
