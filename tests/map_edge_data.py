"""Path-directed inputs for the map insert (LocalMap::addSurfPointCloud, LocalMap.h:591-645) and for the scan pre-filter
(laserMapping::adjustVoxelSize, pcl::VoxelGrid), and plain restatements of their rules (test infrastructure).

The restatements, per point and in Python numbers on purpose:
  cube_coord     int((c + 25.0) / 50.0) + origin, minus one if c + 25.0 < 0 (LocalMap.h:596-605).  A NaN or infinite coordinate is
                 pinned to "outside the window": that is what the conversion gives on x86-64 (INT_MIN), where the reference runs.
  leaf_index     pcl's leaf coordinate floor(float32(x * inv)) with inv = float32(1) / float32(leaf)
  voxel_grid     pcl::VoxelGrid of one cloud: bounding box, the "leaf size too small" pass-through, a dictionary of leaves with
                 sequential float32 sums in arrival order, leaves emitted in ascending (z, y, x)
  PlainMap       the map: cubes filled in arrival order behind their old centroids, every touched cube filtered by voxel_grid;
                 set_origin / shift restated for the window's origin only
Both VoxelGrids are loops over the points and slow: they are for the small families.

A family is a seeded, deterministic function that returns a `Family`: a list of insert clouds, probe queries for the 5-NN (which is
what tells the cube a point was filed in: the search never leaves the query's cube), the resolution and the window set-up.  Every
cube that is probed also receives filler points well away from the site, each in a leaf of its own, so that five neighbours exist.

  cube_faces   points on the cube faces -125 .. 75, one float ulp and 1e-4 m to either side, edges and corners; planeRes 0.2, 0.4
  window_edge  the limits of the 21 x 21 x 11 window, default origin and after set_origin / shift at WINDOW_T
  leaf_faces   the float nearest L * leaf and its two neighbours, two to four points per leaf, seven resolutions
  rounds       inserts that touch exactly 32 / 33 cubes (planeRes 0.2: 32 cubes per round) and 4 / 5 (planeRes 0.05: 4 per round)
  degenerate   an empty cloud, one point, a cloud outside the window, 5 000 copies of a point, 5 000 points alternating between leaves
  non_finite   20 000-point clouds with NaN, +inf, -inf coordinates: lanes 0 and 63, first and last point, a whole wavefront
  cube_escape  400 000 points in one leaf just inside a cube face at |x| = 475: their float centroid lands 0.48 m OUTSIDE the cube
  PREFILTER    clouds for the scan pre-filter: pass-through, the two sides of its threshold, more than 4 096 long leaves, ...

Scan clouds with non-finite points are out of scope for the pre-filter: what pcl does with them depends on is_dense, and the node
removes them before the filter sees the cloud (adapter/laser_mapping_soicp.cpp, removeNaNFromPointCloud).

Nothing here depends on the oracle or on the product's kernels."""
import math

import numpy as np

CUBE, HALF = 50.0, 25.0
W, H, D = 21, 21, 11
DIMS = (W, H, D)
DEFAULT_ORIGIN = (10, 10, 5)
INT32_MAX = 2 ** 31 - 1
WINDOW_T = (130.0, -80.0, 3.0)
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# the plain restatements
# ------------------------------------------------------------------------------------------------------------------------
def cube_coord(c, origin=0):
    """window index of coordinate c along one axis, None for a coordinate that is not finite"""
    c = float(c)
    if math.isnan(c) or math.isinf(c):
        return None
    s = c + 25.0
    i = int(s / 50.0) + origin
    if s < 0:
        i -= 1
    return i


def cube_of_point(p, origin=DEFAULT_ORIGIN):
    """(i, j, k) inside the window, or None"""
    ijk = tuple(cube_coord(p[a], origin[a]) for a in range(3))
    if any(v is None or v < 0 or v >= DIMS[a] for a, v in enumerate(ijk)):
        return None
    return ijk


def cube_linear(ijk):
    return ijk[0] + W * ijk[1] + W * H * ijk[2]


def origin_after_set(t):
    return tuple(-cube_coord(t[a], 0) for a in range(3))


def shift(origin, t):
    """LocalMap::shiftMap for the origin alone: (new origin, position of the sensor's cube in the window)"""
    origin, pos = list(origin), []
    for a in range(3):
        c = cube_coord(t[a], origin[a])
        while c < 3:
            c += 1; origin[a] += 1
        while c >= DIMS[a] - 3:
            c -= 1; origin[a] -= 1
        pos.append(c)
    return tuple(origin), tuple(pos)


def window_limits(origin):
    """[low, high) of the window per axis, as the faces of its first and behind its last cube"""
    return [((0 - origin[a]) * CUBE - HALF, (DIMS[a] - origin[a]) * CUBE - HALF) for a in range(3)]


def leaf_index(x, leaf):
    inv = f32(1.0) / f32(leaf)
    return np.floor((np.asarray(x, f32) * inv).astype(f32)).astype(np.int64)


def voxel_grid(cloud, leaf):
    """pcl::VoxelGrid::applyFilter, float centroids summed in arrival order"""
    cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 3)
    if not len(cloud):
        return cloud.copy()
    inv = f32(1.0) / f32(leaf)
    mn, mx = cloud.min(0), cloud.max(0)
    dx, dy, dz = (int(f32(f32(mx[a] - mn[a]) * inv)) + 1 for a in range(3))
    if dx * dy * dz > INT32_MAX:
        return cloud.copy()  # "Leaf size is too small for the input dataset"
    leaves = {}
    for p, l in zip(cloud, leaf_index(cloud, leaf).tolist()):
        e = leaves.get((l[2], l[1], l[0]))
        if e is None:
            leaves[(l[2], l[1], l[0])] = [p[0], p[1], p[2], 1]
        else:
            e[0] = e[0] + p[0]; e[1] = e[1] + p[1]; e[2] = e[2] + p[2]; e[3] += 1  # np.float32 + np.float32
    out = np.zeros((len(leaves), 3), f32)
    for o, key in enumerate(sorted(leaves)):
        e = leaves[key]
        n = f32(e[3])
        out[o] = (e[0] / n, e[1] / n, e[2] / n)
    return out


class PlainMap:
    """cubes: {(i, j, k) in the window: float32 [n, 3]}"""

    def __init__(self, plane_res, origin=DEFAULT_ORIGIN):
        self.plane_res, self.origin, self.cubes = float(plane_res), tuple(origin), {}

    def set_origin(self, t):
        self.origin = origin_after_set(t)
        return self.origin

    def shift(self, t):
        """only for a map whose cubes all stay inside the window (the families roll the window before they insert)"""
        new, pos = shift(self.origin, t)
        d = tuple(n - o for n, o in zip(new, self.origin))
        moved = {tuple(c[a] + d[a] for a in range(3)): v for c, v in self.cubes.items()}
        self.cubes = {c: v for c, v in moved.items() if all(0 <= c[a] < DIMS[a] for a in range(3))}
        self.origin = new
        return pos

    def add(self, cloud):
        cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 3)
        arrived = {}
        for p in cloud:
            c = cube_of_point(p, self.origin)
            if c is not None:
                arrived.setdefault(c, []).append(p)
        for c, pts in arrived.items():
            old = self.cubes.get(c, np.zeros((0, 3), f32))
            self.cubes[c] = voxel_grid(np.concatenate([old, np.array(pts, f32)]), self.plane_res)
        return sum(len(v) for v in arrived.values())

    def size(self):
        return sum(len(v) for v in self.cubes.values())

    def export(self):
        """ascending linear cube index, a cube's points in its filter's order"""
        keys = sorted(self.cubes, key=cube_linear)
        return np.concatenate([self.cubes[c] for c in keys]) if keys else np.zeros((0, 3), f32)


def float_centroid(pts):
    """sequential float32 sums of one leaf's points, divided by the float count"""
    pts = np.ascontiguousarray(pts, f32)
    return np.array([np.add.accumulate(pts[:, a], dtype=f32)[-1] / f32(len(pts)) for a in range(3)], f32)


# ------------------------------------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------------------------------------
class Family:
    """clouds: the inserts, in order.  probes: 5-NN queries asked after the last insert.  window_t: set_origin(t) and shift(t) before the
    first insert (None: the default origin).  create_res, warmup: the resolution the map is created with and the cloud it receives at that
    resolution before plane_res is set through set_resolution on the live map (None: created at plane_res)."""

    def __init__(self, name, plane_res, clouds, probes, window_t=None, create_res=None, warmup=None, **info):
        self.name, self.plane_res = name, float(plane_res)
        self.warmup = None if warmup is None else np.ascontiguousarray(warmup, f32)
        self.clouds = [np.ascontiguousarray(c, f32).reshape(-1, 3) for c in clouds]
        self.probes = np.ascontiguousarray(probes, f32).reshape(-1, 3)
        self.window_t, self.create_res, self.info = window_t, create_res, info

    def origin(self):
        if self.window_t is None:
            return DEFAULT_ORIGIN
        return shift(origin_after_set(self.window_t), self.window_t)[0]

    def probe_positions(self):
        """window positions of the probes' cubes (for count_5x5), distinct, in order of appearance"""
        seen = []
        for q in self.probes:
            c = cube_of_point(q, self.origin())
            if c is not None and c not in seen:
                seen.append(c)
        return seen


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def around(v):
    """v, one float ulp to either side, 1e-4 m to either side"""
    return [f32(v), up(v), down(v), f32(v + 1e-4), f32(v - 1e-4)]


def _fillers(points, origin, rng, also=()):
    """eight points around the centre of every cube that holds a point of `points` (or of `also`), 1.1 m or more apart per axis: each
    in a leaf of its own at every resolution of this module, 3 m or more from the cube's faces"""
    cubes = []
    for p in list(points) + list(also):
        c = cube_of_point(p, origin)
        if c is not None and c not in cubes:
            cubes.append(c)
    out = []
    for c in cubes:
        centre = np.array([(c[a] - origin[a]) * CUBE for a in range(3)])
        for i in range(8):
            out.append(centre + (i - 3.5) * np.array([1.3, -1.7, 1.1]) + rng.uniform(-0.2, 0.2, 3) + np.array([0.37, 0.41, 0.23]))
    return np.array(out, f32).reshape(-1, 3)


def _probes_of(sites, rng, spread=0.3, exact=True):
    """every site itself (exact) and two points near it"""
    s = np.asarray(sites, f32)
    near = [(s + rng.uniform(-spread, spread, s.shape)).astype(f32) for _ in range(2)]
    return np.concatenate(([s] if exact else []) + near)


CUBE_FACES = (-125.0, -75.0, -25.0, 25.0, 75.0)
Z_FACES = (-25.0, 25.0)  # the other listed faces are cube faces in z too, but the issue keeps z to the two nearest the default origin


def _spaced(rng, n, start):
    """n values from `start` on, 0.9 to 1.5 m apart (irregular: no two probes see two neighbours at one distance)"""
    return start + np.cumsum(rng.uniform(0.9, 1.5, n))


def cube_faces(plane_res, seed=11):
    """One site per axis and face value: the five values of around(face) along the axis, each at an offset of its own along the two
    other axes (separate leaves: the map keeps every one of them as it came), and the five again in ONE leaf column (same offsets:
    the filter merges those of a cube, and a point in the wrong cube moves two centroids).  Then edges and corners: two and three axes on
    faces at once, every combination of the face, one ulp above and one ulp below it (probed from nearby only: the points of one cube
    lie an ulp apart, at one distance from each other)."""
    rng = np.random.default_rng(seed)
    pts, sites = [], []
    for axis in range(3):
        for face in (CUBE_FACES if axis < 2 else Z_FACES):
            base = rng.uniform(-9.0, 9.0, 3)
            base[2] = rng.uniform(-6.0, 6.0)
            o1, o2 = _spaced(rng, 5, base[(axis + 1) % 3]), _spaced(rng, 5, base[(axis + 2) % 3]) * 0.3
            for j, v in enumerate(around(face)):
                p = np.zeros(3); p[axis] = v; p[(axis + 1) % 3] = o1[j]; p[(axis + 2) % 3] = base[(axis + 2) % 3] + o2[j] - o2[0]
                pts.append(p); sites.append((axis, face, j, len(pts) - 1))
            col = math.floor(base[(axis + 2) % 3] / 0.4) * 0.4 + 0.05
            for j, v in enumerate(around(face)):  # the merged column, 4 m away (13 mm apart inside the leaf: no two at one distance from a probe)
                p = np.zeros(3); p[axis] = v; p[(axis + 1) % 3] = o1[0] - 4.03; p[(axis + 2) % 3] = col + 0.013 * j
                pts.append(p)
    corners = []
    combos = [((0, -75.0), (1, -75.0), (2, -25.0)), ((0, 25.0), (1, -25.0), (2, 25.0)), ((0, -125.0), (1, 75.0), (2, -25.0)),
              ((0, -75.0), (1, -75.0)), ((0, 25.0), (1, 75.0)), ((0, -25.0), (2, 25.0)), ((1, -125.0), (2, -25.0)), ((0, 75.0), (1, -25.0))]
    local, local_done, corners_seen = [], set(), []
    for combo in combos:
        free = [a for a in range(3) if a not in [c[0] for c in combo]]
        for k in range(3 ** len(combo)):
            p = np.zeros(3)
            for b, (a, face) in enumerate(combo):
                p[a] = (f32(face), up(face), down(face))[(k // 3 ** b) % 3]
            for a in free:
                p[a] = 3.3 + 1.37 * k  # (a leaf of its own along the free axis)
            corners.append(p)
            # six points 1 to 4 m inside the cube this one fell in, once per cube and corner: a probe near the corner then has six
            # neighbours nearer than any OTHER corner's points (which lie an ulp apart, at one distance from anything far away)
            c = cube_of_point(p)
            if (len(corners_seen), c) not in local_done:
                local_done.add((len(corners_seen), c))
                inward = np.sign(np.array([(c[a] - DEFAULT_ORIGIN[a]) * CUBE for a in range(3)]) - p + 1e-9)
                local.extend(p + inward * (1.0 + 0.5 * i + rng.uniform(0, 0.3, 3)) * np.array([1.0, 0.83, 0.61]) for i in range(6))
        corners_seen.append(combo)
    n_face_points = len(pts)
    pts = np.array(pts + corners, f32)
    fill = _fillers(pts, DEFAULT_ORIGIN, rng)
    cloud = np.concatenate([pts, fill, np.array(local, f32)])
    cloud = cloud[rng.permutation(len(cloud))]
    # a second insert meets the first one's points as old centroids: the same sites, 0.07 m along the first free axis
    again = pts.copy()
    for i, (axis, face, j, at) in enumerate(sites):
        again[at, (axis + 1) % 3] += f32(0.07)
    return Family(f"cube_faces_{plane_res}", plane_res, [cloud, again[:n_face_points]],
                  np.concatenate([_probes_of(pts[:n_face_points], rng), _probes_of(pts[n_face_points:], rng, exact=False)]),
                  sites=sites, points=pts, n_face_points=n_face_points)


def window_edge(shifted, seed=12):
    """Per axis and per limit of the window: the limit, its inward and outward float neighbour, a point 1e-3 m inside and outside, and
    a point in the middle of the outermost cube.  The other two coordinates stay near the sensor."""
    rng = np.random.default_rng(seed + int(shifted))
    t = WINDOW_T if shifted else None
    origin = shift(origin_after_set(t), t)[0] if shifted else DEFAULT_ORIGIN
    centre = np.array(t if shifted else (0.0, 0.0, 0.0))
    pts, limits = [], []
    for axis, (lo, hi) in enumerate(window_limits(origin)):
        for lim, inward in ((lo, 1.0), (hi, -1.0)):
            vals = [f32(lim), up(lim), down(lim), f32(lim + 1e-3), f32(lim - 1e-3), f32(lim + inward * 25.0)]
            o1 = _spaced(rng, len(vals), centre[(axis + 1) % 3] - 4.0)
            for j, v in enumerate(vals):
                p = centre + rng.uniform(-3.0, 3.0, 3)
                p[axis] = v; p[(axis + 1) % 3] = o1[j]
                pts.append(p)
            limits.append((axis, lim, len(pts) - len(vals), len(pts)))
    pts = np.array(pts, f32)
    fill = _fillers(pts, origin, rng)
    cloud = np.concatenate([pts, fill])
    cloud = cloud[rng.permutation(len(cloud))]
    return Family("window_edge_shifted" if shifted else "window_edge", 0.2, [cloud], _probes_of(pts, rng), window_t=t, limits=limits, points=pts)


LEAF_RESOLUTIONS = (0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.8)
SET_ON_LIVE_MAP = (0.15, 0.3)  # these two are reached through set_resolution on a live map, as a resolution change does


def leaf_indices(leaf, axis):
    """about forty leaf indices: small positive and negative ones, zero, around the cube faces at -25, 25 and 75, and far out, where
    x * inv has few fraction bits left (500 m; 250 m in z, whose window is narrower)"""
    far = 250.0 if axis == 2 else 500.0
    L = list(range(-8, 9))
    for c in (-25.0, 25.0, 75.0, far, -far):
        m = int(round(c / leaf))
        L += [m - 1, m, m + 1, m + 2]
    L += [int(round(far / leaf)) - 7, -int(round(far / leaf)) + 7, int(round(123.4 / leaf)), -int(round(123.4 / leaf))]
    return sorted(set(L))


def leaf_triples(leaf):
    """[(axis, L, (below, nearest, above))]: the float nearest L * leaf and its two neighbours"""
    out = []
    for axis in range(3):
        for L in leaf_indices(leaf, axis):
            v = f32(L * leaf)
            out.append((axis, L, (down(v), v, up(v))))
    return out


def leaf_faces(leaf, seed=13):
    """Per triple: the three values along the axis at one (mid-leaf) position of the two other coordinates, and one companion a third of a
    leaf to either side: the two leaves at the face hold two to four points, and a value filed on the wrong side moves both centroids.
    The other two coordinates differ from triple to triple by whole leaves."""
    rng = np.random.default_rng(seed)
    pts, sites = [], []
    for n, (axis, L, vals) in enumerate(leaf_triples(leaf)):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        o1 = (3 * (n % 37) - 50 + 0.5) * leaf
        o2 = (3 * (n // 37) - 7 + 0.5) * leaf
        for v in list(vals) + [f32(vals[1] - 0.33 * leaf), f32(vals[1] + 0.33 * leaf)]:
            p = np.zeros(3); p[axis] = v; p[a1] = o1; p[a2] = o2
            pts.append(p)
        sites.append(pts[-4])
    pts = np.array(pts, f32)
    fill = _fillers(pts, DEFAULT_ORIGIN, rng)
    cloud = np.concatenate([pts, fill])
    cloud = cloud[rng.permutation(len(cloud))]
    second = (pts[::3] + f32(0.25 * leaf) * np.array([0, 1, 0], f32)).astype(f32)  # a later insert meets the centroids as old points
    live = leaf in SET_ON_LIVE_MAP  # (the warm-up: a floor and a wall through the cubes around the origin, filtered at 0.2 first)
    warmup = np.concatenate([np.c_[rng.uniform(-40, 40, (3000, 2)), rng.normal(-1.5, 0.01, 3000)],
                             np.c_[rng.uniform(-40, 40, 1500), rng.normal(10.0, 0.01, 1500), rng.uniform(-1.5, 6.0, 1500)]]) if live else None
    return Family(f"leaf_faces_{leaf}", leaf, [cloud, second], _probes_of(np.array(sites, f32), rng, spread=2.0 * leaf, exact=False),
                  create_res=0.2 if live else None, warmup=warmup, points=pts)


def rounds(plane_res, n_cubes, seed=14):
    """n_cubes cubes of a 6 x 6 block around the origin, 300 points in each, shuffled; and the same cubes again (old centroids)"""
    rng = np.random.default_rng(seed + n_cubes)
    cubes = [(i, j) for j in range(-3, 3) for i in range(-3, 3)][:n_cubes]
    def one():
        parts = [np.c_[rng.uniform(-20, 20, (300, 2)) + np.array([i, j]) * CUBE, rng.normal(0, 0.02, 300) + 0.1 * i] for i, j in cubes]
        p = np.concatenate(parts).astype(f32)
        return p[rng.permutation(len(p))]
    a, b = one(), one()
    return Family(f"rounds_{plane_res}_{n_cubes}", plane_res, [a, b], _probes_of(a[::97], rng), n_cubes=n_cubes)


def degenerate(seed=15):
    rng = np.random.default_rng(seed)
    one = np.array([[3.21, -4.37, 0.93]], f32)
    outside = (rng.uniform(-50, 50, (500, 3)) + np.array([3000.0, -2000.0, 900.0])).astype(f32)
    copies = np.repeat(np.array([[-30.11, 12.07, 2.03]], f32), 5000, 0)
    two = np.array([[7.05, 7.05, 1.05], [7.05, 7.25, 1.05]], f32)
    alternating = (two[np.arange(5000) % 2] + rng.uniform(-0.04, 0.04, (5000, 3))).astype(f32)
    sites = np.concatenate([one, copies[:1], two])
    fill = _fillers(sites, DEFAULT_ORIGIN, rng)
    return Family("degenerate", 0.2, [np.zeros((0, 3), f32), one, outside, copies, alternating, np.zeros((0, 3), f32), fill, one],
                  _probes_of(sites, rng))


def non_finite(seed=16):
    """Two clouds of 20 000 points; in each, NaN, +inf and -inf in x, y or z of about 60 points apiece, and NaN in the first and the
    last point, in lane 0 and lane 63 of a wavefront and in all 64 points of one wavefront"""
    from helpers import noisy_planes_cloud
    rng = np.random.default_rng(seed)
    clouds, bad_rows = [], []
    for k in range(2):
        c = noisy_planes_cloud(20000, rng, offset=(3.0 * k, -2.0 * k, 0.0))
        c = c[rng.permutation(len(c))]
        bad = np.zeros(len(c), bool)
        for value in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(c), 60, replace=False)
            c[rows, rng.integers(0, 3, 60)] = value
            bad[rows] = True
        rows = np.r_[0, len(c) - 1, 64 * 7, 64 * 7 + 63, 64 * 11 + 63, 64 * 13, np.arange(64 * 100, 64 * 101)]
        c[rows, np.arange(len(rows)) % 3] = np.nan
        c[64 * 100 + 5] = np.nan  # all three coordinates
        bad[rows] = True
        clouds.append(c); bad_rows.append(bad)
    good = clouds[0][~bad_rows[0]]
    return Family("non_finite", 0.2, clouds, _probes_of(good[::331], rng), bad_rows=bad_rows)


ESCAPE_N = 400_000


def cube_escape(plane_res, high, seed=1):
    """400 000 points uniform in one leaf 1 to 4 cm inside the cube face x = -475 (high: x = +475): the float sum's spacing grows to
    16 and 32, the addends are rounded to it, and the centroid comes out about 0.48 m beyond the face -- outside the cube it is kept in,
    and beyond the two leaves of margin of the insert's leaf keys.  Then 3 000 points elsewhere in the cube (and fillers in the cube
    across the face), then 50 points in the leaf the centroid landed in (which lies in the cube across the face)."""
    rng = np.random.default_rng(seed)
    sgn = 1.0 if high else -1.0
    big = np.c_[sgn * rng.uniform(474.96, 474.99, ESCAPE_N), rng.uniform(0.01, 0.04, (ESCAPE_N, 2))].astype(f32)
    cent = float_centroid(big)
    second = np.c_[sgn * rng.uniform(430.0, 470.0, 3000), rng.uniform(-20, 20, 3000), rng.normal(0, 0.02, 3000)].astype(f32)
    across = np.array([[sgn * 500.0, 0.0, 0.0]])
    second = np.concatenate([second, _fillers(across, DEFAULT_ORIGIN, rng)])
    leaf_lo = leaf_index(cent, plane_res).astype(np.float64) * plane_res
    third = (leaf_lo + rng.uniform(0.1, 0.9, (50, 3)) * plane_res).astype(f32)
    assert (leaf_index(third, plane_res) == leaf_index(cent, plane_res)).all()
    inside = np.array([sgn * 474.0, 0.02, 0.02])
    probes = np.concatenate([_probes_of(np.array([cent, inside, [sgn * 474.9, 0.0, 0.0], [sgn * 475.1, 0.0, 0.0], [sgn * 476.0, 0.1, 0.1]], f32), rng),
                             np.array([[sgn * 474.999, 0.02, 0.02], [sgn * 475.001, 0.02, 0.02]], f32)])
    return Family(f"cube_escape_{plane_res}_{'high' if high else 'low'}", plane_res, [big, second, third], probes,
                  centroid=cent, inside=inside.astype(f32), face=sgn * 475.0, sign=sgn)


SMALL_FAMILIES = {
    "cube_faces_0.2": lambda: cube_faces(0.2),
    "cube_faces_0.4": lambda: cube_faces(0.4),
    "window_edge": lambda: window_edge(False),
    "window_edge_shifted": lambda: window_edge(True),
    **{f"leaf_faces_{r}": (lambda r=r: leaf_faces(r)) for r in LEAF_RESOLUTIONS},
    "rounds_0.2_32": lambda: rounds(0.2, 32),
    "rounds_0.2_33": lambda: rounds(0.2, 33),
    "rounds_0.05_4": lambda: rounds(0.05, 4),
    "rounds_0.05_5": lambda: rounds(0.05, 5),
    "degenerate": degenerate,
    "non_finite": non_finite,
}
ESCAPE_FAMILIES = {f"cube_escape_{r}_{'high' if h else 'low'}": (lambda r=r, h=h: cube_escape(r, h)) for r in (0.05, 0.1, 0.2) for h in (False, True)}
FAMILIES = {**SMALL_FAMILIES, **ESCAPE_FAMILIES}
# the families that also run with every round laid out by the host, with the sort-based first stage and on the host map
EVERY_MODE = [n for n in SMALL_FAMILIES if n.split("_")[0] in ("cube", "window", "non", "rounds")]
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------------------------------
# clouds for the scan pre-filter
# ------------------------------------------------------------------------------------------------------------------------
class Cloud:
    """one call of so_icp_prefilter_scan(cloud, auto, line_res, plane_res)"""

    def __init__(self, name, cloud, plane_res=0.4, **info):
        self.name, self.cloud, self.plane_res, self.line_res, self.info = name, np.ascontiguousarray(cloud, f32), float(plane_res), plane_res / 2, info


def bounding_box_leaves(cloud, leaf):
    """pcl's dx, dy, dz: (int64)((max - min) * inv) + 1 in float arithmetic"""
    inv = f32(1.0) / f32(leaf)
    mn, mx = cloud.min(0), cloud.max(0)
    return tuple(int(f32(f32(mx[a] - mn[a]) * inv)) + 1 for a in range(3))


def leaf_sizes(cloud, leaf):
    """points per occupied leaf"""
    return np.unique(leaf_index(cloud, leaf), axis=0, return_counts=True)[1]


def _pass_through(seed=21):
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform(-5, 5, (2000, 3)), [[900.0, 900.0, 900.0]], [[-900.0, -900.0, -900.0]]]).astype(f32)
    return c[rng.permutation(len(c))]


def _box(n_leaves, seed=22):
    """2 000 points in +-5 m (several to a 0.2 m leaf) and two corner points that set the bounding box to n_leaves leaves a side"""
    rng = np.random.default_rng(seed)
    lo = -129.0
    hi = lo + (n_leaves - 0.5) * 0.2
    c = np.concatenate([rng.uniform(-5, 5, (2000, 3)) * [1, 1, 0.1], [[lo, lo, lo]], [[hi, hi, hi]]]).astype(f32)
    return c[rng.permutation(len(c))]


def _long_leaves(seed=23):
    """4 200 leaves (0.2 m, every other leaf of a sheet 80 leaves wide) of 65 to 70 points and 2 000 leaves of 1 to 9 points, shuffled"""
    rng = np.random.default_rng(seed)
    parts = []
    for n in range(6200):
        i, j = n % 80, n // 80
        centre = np.array([(2 * i - 80 + 0.5) * 0.2, (2 * j - 78 + 0.5) * 0.2, 0.1])
        m = int(rng.integers(65, 71)) if n < 4200 else int(rng.integers(1, 10))
        parts.append(centre + rng.uniform(-0.08, 0.08, (m, 3)))
    c = np.concatenate(parts).astype(f32)
    return c[rng.permutation(len(c))]


def _leaves_of_64(seed=24):
    """leaves of exactly 63, 64, 65 and 66 points (the limit of the one-thread sum is 64), five of each, among short ones"""
    rng = np.random.default_rng(seed)
    parts = []
    for n, m in enumerate([63, 64, 65, 66] * 5 + [1, 2, 3, 17] * 30):
        centre = np.array([(2 * (n % 12) - 11 + 0.5) * 0.4, (2 * (n // 12) - 9 + 0.5) * 0.4, 0.2])
        parts.append(centre + rng.uniform(-0.15, 0.15, (m, 3)))
    c = np.concatenate(parts).astype(f32)
    return c[rng.permutation(len(c))]


def _leaf_faces_cloud(leaf):
    """the leaf_faces points within 60 m of the origin: VoxelGrid works relative to the cloud's own min_b = floor(min * inv)"""
    p = family(f"leaf_faces_{leaf}").info["points"]
    return p[(np.abs(p) < 60.0).all(1)]


PREFILTER = {
    "pass_through": lambda: Cloud("pass_through", _pass_through(), 0.4),
    "pass_through_0.8": lambda: Cloud("pass_through_0.8", _pass_through(), 0.8),
    "box_1290": lambda: Cloud("box_1290", _box(1290), 0.2, side=1290),
    "box_1291": lambda: Cloud("box_1291", _box(1291), 0.2, side=1291),
    "long_leaves": lambda: Cloud("long_leaves", _long_leaves(), 0.2),
    "leaves_of_64": lambda: Cloud("leaves_of_64", _leaves_of_64(), 0.4),
    "leaf_faces_0.2": lambda: Cloud("leaf_faces_0.2", _leaf_faces_cloud(0.2), 0.2),
    "leaf_faces_0.4": lambda: Cloud("leaf_faces_0.4", _leaf_faces_cloud(0.4), 0.4),
    "single_point": lambda: Cloud("single_point", np.array([[1.5, -2.5, 0.5]], f32), 0.4),
    "identical_points": lambda: Cloud("identical_points", np.repeat(np.array([[1.5, -2.5, 0.5]], f32), 3000, 0), 0.4),
}
PASS_THROUGH = ("pass_through", "pass_through_0.8", "box_1291")


def prefilter_cloud(name):
    if ("pf", name) not in _cache:
        _cache[("pf", name)] = PREFILTER[name]()
    return _cache[("pf", name)]
