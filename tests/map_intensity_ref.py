"""Four-channel restatements of the scan pre-filter's and the map insert's pcl::VoxelGrid<pcl::PointXYZI> -- x y z and the INTENSITY,
which PCL averages per leaf like every other field (downsample_all_data, its default) -- and the seeded inputs of the intensity tests.
Test infrastructure only; nothing here depends on the oracle or on the product's kernels.

PCL is not available to this project's tests, so the rules are restated from pcl::CentroidPoint<PointXYZI>: AccumulatorXYZ holds a
Vector3f sum, AccumulatorIntensity a float sum, both are divided by the point count converted to float.
  voxel_grid_xyzi  map_edge_data.voxel_grid with a fourth column: the same bounding box, pass-through, leaves and order (all from x y z
                   alone); per leaf the sequential float32 sum of the members' intensities in arrival order, divided by float32(count)
  PlainMapI        map_edge_data.PlainMap on [n, 4] points: cubes by x y z, old centroids first, then the new points in arrival order
The cube, leaf and window rules are map_edge_data's own functions, imported, not copied.

Inputs (insert_input): three inserts into a map at planeRes 0.2, as float32 records [n, 8] (stride 32: x y z, a marker at byte 12 that
nothing may read, the intensity at byte 16, markers behind it).  Every insert places, for each size of LEAF_SIZES, leaves whose member
count -- the cube's old centroid, if the leaf has one, and the new points -- is exactly that size: the sizes on both sides of every
limit of the summing kernels (one thread up to 4 and up to 16 members, one wavefront up to 64, one workgroup up to 4 096, and the
overflow beyond, which repeats the round on the sort path; there: one thread up to 64, one wavefront beyond).  Intensities are seeded
floats in [0, 255]."""
import numpy as np

from map_edge_data import DEFAULT_ORIGIN, INT32_MAX, PlainMap, cube_linear, cube_of_point, leaf_index

f32 = np.float32
LEAF = 0.2
LEAF_SIZES = (1, 2, 3, 4, 5, 16, 17, 64, 65, 100, 1000, 4096)
OVERFLOW_SIZE = 4097
# member count -> the kernel that sums the leaf on the hashed path
CLASSES = ((1, 1), (2, 4), (5, 16), (17, 64), (65, 4096), (4097, 1 << 30))


def size_class(n):
    return next(k for k, (lo, hi) in enumerate(CLASSES) if lo <= n <= hi)


def class_histogram(sizes):
    h = [0] * len(CLASSES)
    for n in sizes:
        h[size_class(int(n))] += 1
    return h


def voxel_grid_xyzi(cloud, leaf, sizes=None):
    """pcl::VoxelGrid<PointXYZI>::applyFilter on float32 [n, 4]; sizes: a list that receives the member count of every output leaf"""
    cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 4)
    if not len(cloud):
        return cloud.copy()
    inv = f32(1.0) / f32(leaf)
    xyz = cloud[:, :3]
    mn, mx = xyz.min(0), xyz.max(0)
    dx, dy, dz = (int(f32(f32(mx[a] - mn[a]) * inv)) + 1 for a in range(3))
    if dx * dy * dz > INT32_MAX:
        if sizes is not None:
            sizes.extend([1] * len(cloud))
        return cloud.copy()  # "Leaf size is too small for the input dataset"
    leaves = {}
    for p, l in zip(cloud, leaf_index(xyz, leaf).tolist()):
        e = leaves.get((l[2], l[1], l[0]))
        if e is None:
            # (the accumulators start at zero: 0 + p, which is p except for the sign of a zero)
            leaves[(l[2], l[1], l[0])] = [f32(0) + p[0], f32(0) + p[1], f32(0) + p[2], f32(0) + p[3], 1]
        else:
            e[0] = e[0] + p[0]; e[1] = e[1] + p[1]; e[2] = e[2] + p[2]; e[3] = e[3] + p[3]; e[4] += 1  # np.float32 + np.float32
    out = np.zeros((len(leaves), 4), f32)
    with np.errstate(invalid="ignore"):
        for o, key in enumerate(sorted(leaves)):
            e = leaves[key]
            n = f32(e[4])
            out[o] = (e[0] / n, e[1] / n, e[2] / n, e[3] / n)
            if sizes is not None:
                sizes.append(e[4])
    return out


class PlainMapI(PlainMap):
    """cubes: {(i, j, k) in the window: float32 [n, 4]}; group_sizes: member counts of the leaves of the cubes the last add() touched;
    set_origin and shift are PlainMap's (they move whole cubes)"""

    def __init__(self, plane_res, origin=DEFAULT_ORIGIN):
        super().__init__(plane_res, origin)
        self.group_sizes = []

    def add(self, cloud):
        cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 4)
        arrived = {}
        for p in cloud:
            c = cube_of_point(p[:3], self.origin)
            if c is not None:
                arrived.setdefault(c, []).append(p)
        self.group_sizes = []
        for c, pts in arrived.items():
            old = self.cubes.get(c, np.zeros((0, 4), f32))
            self.cubes[c] = voxel_grid_xyzi(np.concatenate([old, np.array(pts, f32)]), self.plane_res, self.group_sizes)
        return sum(len(v) for v in arrived.values())

    def export(self):
        """ascending linear cube index, a cube's points in its filter's order"""
        keys = sorted(self.cubes, key=cube_linear)
        return np.concatenate([self.cubes[c] for c in keys]) if keys else np.zeros((0, 4), f32)

    def records(self):
        """the export as 32-byte records: x y z, 1.0f, intensity, zero padding (uint8 [n, 32])"""
        return xyzi_records(self.export())


def xyzi_records(xyzi, with_intensity=True):
    xyzi = np.ascontiguousarray(xyzi, f32).reshape(-1, 4)
    rec = np.zeros((len(xyzi), 8), f32)
    rec[:, :3] = xyzi[:, :3]
    if with_intensity:
        rec[:, 3] = 1.0
        rec[:, 4] = xyzi[:, 3]
    return rec.view(np.uint8).reshape(len(xyzi), 32)


def to_records(xyzi):
    """float32 [n, 8] input records: x y z, marker, intensity, markers"""
    xyzi = np.ascontiguousarray(xyzi, f32).reshape(-1, 4)
    rec = np.empty((len(xyzi), 8), f32)
    rec[:, :3] = xyzi[:, :3]
    rec[:, 3] = 777.0
    rec[:, 4] = xyzi[:, 3]
    rec[:, 5:] = (555.0, 444.0, 333.0)
    return rec


def sorted_by_xyz(rec):
    """uint8 [n, stride] records in ascending (z, y, x) of their first three floats"""
    xyz = np.ascontiguousarray(rec[:, :12]).view(f32).reshape(-1, 3)
    return rec[np.lexsort(xyz.T)]


def distinct_xyz(xyzi):
    xyz = np.ascontiguousarray(np.asarray(xyzi, f32)[:, :3])
    return len(np.unique(xyz.view(np.uint32).reshape(-1, 3), axis=0)) == len(xyz)


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
class Input:
    """clouds: [n, 4] per insert; site_of: per insert, the site number of every point (-1: background); sites: {number: target size};
    plane_res: per insert (a change between inserts is a set_resolution on the live map)"""

    def __init__(self, name, clouds, site_of, sites, plane_res):
        self.name, self.clouds, self.site_of, self.sites, self.plane_res = name, clouds, site_of, sites, plane_res


def site_centre(k):
    """leaf centres three leaves apart on a sheet inside the cube around the origin (its own leaf at 0.2 and at 0.4)"""
    i, j = k % 40, k // 40
    return np.array([(3 * i - 60 + 0.5) * LEAF, (3 * j - 40 + 0.5) * LEAF, 0.5 * LEAF + 1.0])


def _members(rng, k, m):
    xyz = site_centre(k) + rng.uniform(-0.07, 0.07, (m, 3))
    return np.c_[xyz, rng.uniform(0.0, 255.0, m)].astype(f32)


def insert_input(overflow=False, seed=31):
    """Three inserts.  Set A arrives in insert 0 with `size` new points per leaf and in inserts 1 and 2 with size - 1 (the old centroid
    is the first member; a leaf of size 1 receives nothing and passes through); set B arrives in insert 1 and returns in insert 2; set C
    (the sizes up to 100) arrives in insert 2.  overflow: a leaf of 4 097 members in inserts 0 and 1."""
    rng = np.random.default_rng(seed + int(overflow))
    sizes_a = [s for s in LEAF_SIZES for _ in range(3 if s <= 100 else 1)] + ([OVERFLOW_SIZE] if overflow else [])
    sizes_b = [s for s in LEAF_SIZES if s <= 1000 or not overflow]
    sizes_c = [s for s in LEAF_SIZES if s <= 100]
    sites, k0 = {}, 0
    sets = []
    for sizes in (sizes_a, sizes_b, sizes_c):
        sets.append(list(range(k0, k0 + len(sizes))))
        sites.update({k0 + n: s for n, s in enumerate(sizes)})
        k0 += len(sizes)
    clouds, site_of = [], []
    for step in range(3):
        parts, ids = [], []
        for first, members in enumerate(sets[:step + 1]):
            fresh = first == step
            for k in members:
                m = sites[k] if fresh else sites[k] - 1
                if sites[k] == OVERFLOW_SIZE and step == 2:
                    m = 3  # (the third insert stays on the hashed path)
                if m:
                    parts.append(_members(rng, k, m)); ids.append(np.full(m, k))
        cloud, ids = np.concatenate(parts), np.concatenate(ids)
        order = rng.permutation(len(cloud))
        clouds.append(cloud[order]); site_of.append(ids[order])
    return Input("overflow" if overflow else "classes", clouds, site_of, sites, [LEAF] * 3)


def many_cubes_input(n_cubes=33, seed=33):
    """two inserts over n_cubes cubes (32 make a round at planeRes 0.2), 150 points each in clusters of a few to a leaf"""
    rng = np.random.default_rng(seed)
    cubes = [(i, j) for j in range(-3, 3) for i in range(-3, 3)][:n_cubes]

    def one():
        parts = []
        for i, j in cubes:
            c = rng.uniform(-20, 20, (50, 2)) + np.array([i, j]) * 50.0
            xy = np.repeat(c, 3, 0) + rng.uniform(-0.05, 0.05, (150, 2))
            parts.append(np.c_[xy, rng.normal(0, 0.02, 150) + 0.1 * i, rng.uniform(0.0, 255.0, 150)])
        p = np.concatenate(parts).astype(f32)
        return p[rng.permutation(len(p))]
    clouds = [one(), one()]
    return Input(f"cubes_{n_cubes}", clouds, [np.full(len(c), -1) for c in clouds], {}, [LEAF] * 2)


def retable_input(seed=35):
    """an insert at 0.2, then two at 0.4 (set_resolution between them: the cell tables are rebuilt over the resident points, and the
    next insert re-filters the cube, several old centroids to a leaf, in the old grid's order)"""
    rng = np.random.default_rng(seed)

    def sheet(n):
        return np.c_[rng.uniform(-6, 6, (n, 2)), rng.normal(-1.5, 0.02, n), rng.uniform(0.0, 255.0, n)].astype(f32)
    base = insert_input(seed=seed)
    clouds = [np.concatenate([base.clouds[0][base.site_of[0] < 20], sheet(6000)]), np.concatenate([base.clouds[1][base.site_of[1] < 20], sheet(3000)]),
              sheet(2000)]
    return Input("retable", clouds, [np.full(len(c), -1) for c in clouds], {}, [0.2, 0.4, 0.4])


def non_finite_input(seed=31):
    """the `classes` input with a NaN intensity in one leaf of 3 and one of 100 members, +inf in another of each (first insert)"""
    inp = insert_input(seed=seed)
    clouds = [c.copy() for c in inp.clouds]
    poisoned = {}
    for size in (3, 100):
        ks = [k for k, s in inp.sites.items() if s == size][:2]
        for k, v in zip(ks, (np.nan, np.inf)):
            rows = np.nonzero(inp.site_of[0] == k)[0]
            clouds[0][rows[len(rows) // 2], 3] = v
            poisoned[k] = v
    out = Input("non_finite", clouds, inp.site_of, inp.sites, inp.plane_res)
    out.poisoned = poisoned
    return out


INPUTS = {"classes": insert_input, "overflow": lambda: insert_input(True), "cubes_33": many_cubes_input, "retable": retable_input,
          "non_finite": non_finite_input}
_cache = {}


def get_input(name):
    if name not in _cache:
        _cache[name] = INPUTS[name]()
    return _cache[name]


def reference(name):
    """(PlainMapI after every insert as [n, 4] exports, class histogram of every insert's touched leaves) of an input -- computed once"""
    key = ("ref", name)
    if key not in _cache:
        inp = get_input(name)
        pm, exports, hists = PlainMapI(inp.plane_res[0]), [], []
        for cloud, res in zip(inp.clouds, inp.plane_res):
            pm.plane_res = float(res)
            pm.add(cloud)
            exports.append(pm.export()); hists.append(class_histogram(pm.group_sizes))
        _cache[key] = (exports, hists)
    return _cache[key]


def with_intensity_column(cloud, seed):
    """float32 [n, 3] -> [n, 4] with seeded intensities in [0, 255]"""
    cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 3)
    return np.c_[cloud, np.random.default_rng(seed).uniform(0.0, 255.0, len(cloud))].astype(f32)


def prefilter_reference(name):
    """(the map_edge_data pre-filter cloud `name` with an intensity column [n, 4], its voxel_grid_xyzi at the cloud's planeRes) -- once"""
    from map_edge_data import prefilter_cloud
    key = ("pf", name)
    if key not in _cache:
        pc = prefilter_cloud(name)
        xyzi = with_intensity_column(pc.cloud, 7)
        _cache[key] = (xyzi, voxel_grid_xyzi(xyzi, pc.plane_res))
    return _cache[key]
